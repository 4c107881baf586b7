// Host-code checker for libbote_hip.so's host-only translation unit
// (fantoch_amd/csrc/bote_host.cpp), built with ASan + UBSan by
// tests/test_sanitize.py: colex ranks, the binomial table, the group walk and
// its chunk/shard cuts, quad layouts, the low table, fast-path eligibility,
// the sweep planning (fast_limits, score_bands, the compiled-in objective set,
// slot_exists_n, chunk_states, the seed's sample plan, sweep_runlen) and
// result-block unpacking, each against a direct restatement, and the C ABI's
// argument checks against their codes, texts and order.  Prints
// "host ok" on success; any failed check exits 1.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../fantoch_amd/csrc/bote_host.hpp"

using namespace bote::host;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// Direct restatement of a cost-balanced cut: walk every group of [rb, re)
// with per-group binomials (no table, no cache), cost ceil(len / 64) + gc.
static std::vector<uint64_t> direct_chunks(uint32_t ns, uint32_t n, uint32_t nc, uint64_t rb, uint64_t re,
                                           uint32_t nchunks) {
  std::vector<uint64_t> out;
  const uint32_t F = n - 3;
  std::vector<uint32_t> p(n);
  colex_unrank(rb, n, ns, p.data());
  std::vector<uint32_t> q(p.begin() + 3, p.end());
  std::vector<uint64_t> gb, gl;
  std::vector<double> gc;
  double total = 0;
  const double G = group_cost(nc);
  for (;;) {
    uint64_t base = 0;
    for (uint32_t k = 0; k < F; ++k) base += binom_u64(q[k], k + 4);
    const uint64_t g = binom_u64(q[0], 3);
    const uint64_t b = std::max(base, rb), e = std::min(base + g, re);
    if (b >= re) break;
    if (e > b) {
      gb.push_back(b);
      gl.push_back(e - b);
      gc.push_back((double)((e - b + 63) / 64) + G);
      total += gc.back();
    }
    if (e >= re) break;
    uint32_t k = 0;
    while (k < F && q[k] + 1 >= (k + 1 < F ? q[k + 1] : ns)) ++k;
    if (k == F) break;
    ++q[k];
    for (uint32_t j = 0; j < k; ++j) q[j] = 3 + j;
  }
  out.push_back(rb);
  double cum = 0;
  size_t i = 0;
  for (uint32_t c = 1; c < nchunks; ++c) {
    const double tgt = total * c / nchunks;
    while (i < gc.size() && cum + gc[i] <= tgt) cum += gc[i++];
    uint64_t bnd = re;
    if (i < gc.size()) bnd = gb[i] + (uint64_t)((tgt - cum) / gc[i] * (double)gl[i]);
    out.push_back(std::max(out.back(), std::min(bnd, re)));
  }
  out.push_back(re);
  return out;
}

static void check_binomials() {
  for (uint32_t ns : {1u, 5u, 20u, 64u, 128u, 130u, 256u}) {
    const uint32_t n = 16;
    const auto t = binom_table(ns, n);
    for (uint32_t m = 0; m <= ns; ++m)
      for (uint32_t k = 0; k <= n; ++k) CHECK(t[(size_t)m * (n + 1) + k] == binom_u64(m, k));
  }
  CHECK(binom_u64(64, 7) == 621216192ull);
  CHECK(binom_u64(128, 6) == 5423611200ull);
  CHECK(binom_u64(256, 16) == 0);  // overflow is 0
}

static void check_unrank() {
  std::mt19937_64 rng(7);
  const uint32_t shapes[][2] = {{20, 5}, {64, 7}, {128, 6}, {17, 13}, {5, 5}};
  for (auto& sh : shapes) {
    const uint32_t ns = sh[0], n = sh[1];
    const uint64_t total = binom_u64(ns, n);
    std::vector<uint32_t> p(n);
    for (int i = 0; i < 2000; ++i) {
      const uint64_t r = i < 2 ? (i == 0 ? 0 : total - 1) : rng() % total;
      CHECK(colex_unrank(r, n, ns, p.data()));
      for (uint32_t j = 1; j < n; ++j) CHECK(p[j - 1] < p[j]);
      CHECK(p[n - 1] < ns);
      CHECK(colex_rank(p.data(), n) == r);
    }
    CHECK(!colex_unrank(total, n, ns, p.data()));
  }
}

static void check_walk() {
  // the bench workload: R=64 n=7, every group of the rank space
  const uint32_t ns = 64, n = 7, nc = 64;
  const uint64_t total = binom_u64(ns, n);
  const auto t0 = std::chrono::steady_clock::now();
  auto w = walk_groups(ns, n, nc, 0, total);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  CHECK(w != nullptr);
  if (!w) return;
  std::printf("walk R=64 n=7: %zu groups in %.1f ms\n", w->start.size(), ms);
  CHECK(w->start.size() == binom_u64(ns - 3, n - 3));
  uint64_t at = 0;
  for (size_t i = 0; i < w->start.size(); ++i) {
    CHECK(w->start[i] == at);
    CHECK(w->len[i] > 0);
    at += w->len[i];
  }
  CHECK(at == total);
  // cuts: against the direct restatement, over the full range and sub-ranges
  // (a shard's chunk table cut from the shared full-range walk)
  for (uint32_t parts : {1u, 2u, 3u, 8u, 9u}) {
    const auto a = cut_chunks(*w, 0, total, parts), b = direct_chunks(ns, n, nc, 0, total, parts);
    CHECK(a == b);
    CHECK(a.size() == parts + 1 && a.front() == 0 && a.back() == total);
    for (size_t i = 1; i < a.size(); ++i) CHECK(a[i - 1] <= a[i]);
  }
  const auto sh = cut_chunks(*w, 0, total, 8);
  for (size_t i = 0; i + 1 < sh.size(); ++i) {
    const auto a = cut_chunks(*w, sh[i], sh[i + 1], 256);
    const auto b = direct_chunks(ns, n, nc, sh[i], sh[i + 1], 256);
    CHECK(a == b);
    auto ws = walk_groups(ns, n, nc, sh[i], sh[i + 1]);
    CHECK(ws && cut_chunks(*ws, sh[i], sh[i + 1], 256) == a);
  }
  // ranges that split a group, tiny ranges, one-config ranges
  std::mt19937_64 rng(11);
  for (int i = 0; i < 200; ++i) {
    uint64_t b = rng() % total, e = std::min(total, b + 1 + rng() % 5000);
    const auto a = cut_chunks(*w, b, e, 1 + rng() % 40);
    const uint32_t k = (uint32_t)a.size() - 1;
    CHECK(a == direct_chunks(ns, n, nc, b, e, k));
  }
  CHECK(cut_chunks(*w, 5, 5, 4).empty());
  // the guided table of a full launch (4,096 waves, 32 chunks per wave, 3
  // tail rounds): ascending, covering [0, total), the base-size chunks then
  // 3 rounds of 4,096 chunks of 1/2, 1/4, 1/8 of the base size
  {
    const uint32_t nw = 4096, cpw = 32;
    const auto g = cut_chunks_guided(*w, 0, total, nw * cpw, nw, 3);
    CHECK(g.front() == 0 && g.back() == total);
    for (size_t i = 1; i < g.size(); ++i) CHECK(g[i - 1] <= g[i]);
    const size_t nch = g.size() - 1;
    CHECK(nch > 3 * (size_t)nw && nch < (size_t)nw * cpw + 3 * nw);
    auto span = [&](size_t i) { return (double)(g[i + 1] - g[i]); };
    double head = 0, t1 = 0, t3 = 0;
    for (size_t i = 0; i < nch - 3 * nw; ++i) head += span(i);
    for (size_t i = nch - 3 * nw; i < nch - 2 * nw; ++i) t1 += span(i);
    for (size_t i = nch - nw; i < nch; ++i) t3 += span(i);
    head /= (double)(nch - 3 * nw);
    t1 /= nw;
    t3 /= nw;
    std::printf("guided chunks: %zu, mean ranks per chunk: base %.0f, tail 1/2 %.0f, tail 1/8 %.0f\n", nch, head, t1, t3);
    CHECK(t1 < 0.7 * head && t3 < 0.25 * head);
    // no tail: the equal-cost table; too few chunks per wave for a tail: the same
    CHECK(cut_chunks_guided(*w, 0, total, nw * cpw, 0, 3) == cut_chunks(*w, 0, total, nw * cpw));
    CHECK(cut_chunks_guided(*w, 0, total, nw * 8, nw, 3) == cut_chunks(*w, 0, total, nw * 8));
    // a shard's table
    const auto sg = cut_chunks_guided(*w, sh[3], sh[4], nw * 22, nw, 3);
    CHECK(sg.front() == sh[3] && sg.back() == sh[4]);
    for (size_t i = 1; i < sg.size(); ++i) CHECK(sg[i - 1] <= sg[i]);
  }
  // a walk does not serve a range it does not cover
  auto part = walk_groups(ns, n, nc, 1000, 2000);
  CHECK(part && part->covers(1000, 2000) && !part->covers(999, 2000));
  CHECK(cut_chunks(*part, 0, 2000, 4).empty());
  // R=128 n=6 (config 5) walk
  auto w2 = walk_groups(128, 6, 128, 0, binom_u64(128, 6));
  CHECK(w2 && w2->start.size() == binom_u64(125, 3));
  CHECK(walk_groups(64, 3, 64, 0, 10) == nullptr);  // n < 4: no groups
  CHECK(group_utilisation(64, 7) > 0.9);
}

static void check_layouts() {
  const uint32_t R = 9;
  std::vector<uint16_t> lat(R * R);
  for (uint32_t i = 0; i < R; ++i)
    for (uint32_t j = 0; j < R; ++j) lat[i * R + j] = i == j ? 0 : (uint16_t)(10 + 3 * i + j);
  const uint32_t rows[] = {4, 1, 7, 0, 8};
  uint32_t quads = 0, stride = 0;
  const auto m = quad_layout(lat.data(), R, rows, 5, 4, quads, stride);
  CHECK(quads == 2);
  CHECK(stride == 6);  // >= quads + 1, an odd number of 16-B units
  CHECK(m.size() == (size_t)R * stride * 4);
  for (uint32_t t = 0; t < R; ++t)
    for (uint32_t c = 0; c < stride * 4; ++c)
      CHECK(m[t * stride * 4 + c] == (c < 5 ? (uint16_t)(lat[rows[c] * R + t] << 4) : 0));
  for (uint32_t q = 0; q < 300; ++q) {
    const uint32_t s = quad_stride(q);
    CHECK(s >= q + 1 && s % 2 == 0 && (s / 2) % 2 == 1 && s <= q + 4);
  }
  CHECK(quad_stride(16) == 18 && quad_stride(32) == 34);
  const auto lt = low_table(10);
  CHECK(lt.size() == binom_u64(10, 3));
  for (size_t i = 0; i < lt.size(); ++i) {
    const uint32_t p[3] = {lt[i] & 0xFF, (lt[i] >> 8) & 0xFF, lt[i] >> 16};
    CHECK(colex_rank(p, 3) == i);
  }
  std::vector<uint32_t> srv(R);
  for (uint32_t i = 0; i < R; ++i) srv[i] = i;
  CHECK(fast_eligible(lat.data(), R, srv.data(), R, R, false));
  CHECK(!fast_eligible(lat.data(), R, srv.data(), R, R, true));
  CHECK(!fast_eligible(lat.data(), R, srv.data(), R, 1, false));
  std::swap(srv[0], srv[1]);
  CHECK(!fast_eligible(lat.data(), R, srv.data(), R, R, false));
  std::swap(srv[0], srv[1]);
  lat[2 * R + 3] = 0;  // a zero server-server latency
  CHECK(!fast_eligible(lat.data(), R, srv.data(), R, R, false));
  lat[2 * R + 3] = 4096;  // above the packed range
  CHECK(!fast_eligible(lat.data(), R, srv.data(), R, R, false));
}

static void check_unpack() {
  const uint32_t n_obj = 3, kp = 128, K = 5;
  std::vector<uint8_t> blk((size_t)n_obj * kp * 16 + 16, 0xFF);
  auto* r = (TopkRecord*)blk.data();
  for (uint32_t o = 0; o < n_obj; ++o)
    for (uint32_t i = 0; i < o + 3; ++i) r[o * kp + i] = TopkRecord{100u * o + i, 7u * i};
  uint64_t* cnt = (uint64_t*)(blk.data() + (size_t)n_obj * kp * 16);
  cnt[0] = 42;
  cnt[1] = 0xABCDEF;
  std::vector<TopkRecord> out(n_obj * K);
  uint32_t c[3];
  uint64_t valid = 0, dig = 0;
  unpack_result(blk.data(), n_obj, K, kp, out.data(), c, &valid, &dig);
  CHECK(valid == 42 && dig == 0xABCDEF);
  for (uint32_t o = 0; o < n_obj; ++o) {
    CHECK(c[o] == std::min(K, o + 3));
    for (uint32_t i = 0; i < K; ++i)
      CHECK(i < c[o] ? (out[o * K + i].key == 100u * o + i && out[o * K + i].rank == 7u * i)
                     : (out[o * K + i].key == ~0ull && out[o * K + i].rank == ~0ull));
  }
  unpack_result(blk.data(), n_obj, K, kp, nullptr, nullptr, nullptr, nullptr);  // all outputs optional
}

// The group geometry choice (bote_capi_sweep.hip): client-line coverage up to 8
// per wave first, then waves per CU, then more lines, then the smaller size;
// checked on the three measured R=128/R=64 cases.
static void check_geometry() {
  // R=64 n=7: 256 x 4 per CU vs 512 x 2, both 16 lines -> 256
  CHECK(pick_group_geometry(256, 4, 16, 0, 0, 0));
  CHECK(!pick_group_geometry(512, 2, 16, 256, 4, 16));
  // R=128 10 keys: 256 x 3 with 4 lines vs 512 x 2 with 16 -> 512
  CHECK(pick_group_geometry(512, 2, 16, 256, 3, 4));
  // extended keys: 256 x 3 without lines, 512 x 1, 768 x 1 (16 lines) -> 768
  CHECK(pick_group_geometry(512, 1, 16, 256, 3, 0));
  CHECK(pick_group_geometry(768, 1, 16, 512, 1, 16));
  CHECK(!pick_group_geometry(1024, 0, 16, 768, 1, 16));  // does not fit
  CHECK(!pick_group_geometry(256, 0, 0, 0, 0, 0));
}

// Chunks per wave (sweep_chunks): the cap on full sweeps, fewer on shards.
static void check_chunks_per_wave() {
  // R=64 n=7 on 4096 waves, 64 clients (group cost 0.64 steps)
  CHECK(chunks_per_wave(621216192ull, 4096, 64, 32) == 32);
  CHECK(chunks_per_wave(621216192ull / 8, 4096, 64, 32) == 22);
  CHECK(chunks_per_wave(621216192ull / 64, 4096, 64, 32) == 8);
  CHECK(chunks_per_wave(1000, 4096, 64, 32) == 4);
  CHECK(chunks_per_wave(5423611200ull, 4096, 128, 32) == 32);
  CHECK(chunks_per_wave(1ull << 40, 0, 64, 32) == 4);
  CHECK(chunks_per_wave(1ull << 40, 4096, 64, 2) == 2);
}

// ------------------------------------------------------ sweep planning ---
// The arithmetic of bote_sweep_create_keys as it stood in the C ABI before it
// moved to bote_host.cpp, restated inequality by inequality.
struct LimitsRef {
  bool s32, v32, bins, keys32;
};
static LimitsRef limits_ref(uint64_t maxlat, uint32_t nc, uint32_t n) {
  const uint64_t two32 = 1ull << 32, two24 = 1ull << 24, two16 = 1ull << 16;
  const uint64_t cnt = nc > n ? nc : n, a = 2 * maxlat, key = 16 * maxlat + 15;
  LimitsRef r;
  r.s32 = cnt * a * a < two32 && 3ull * nc * maxlat < two24;
  r.v32 = r.s32 && cnt * maxlat < two16;
  r.bins = nc < 256 && (uint64_t)nc * key < two24 && (uint64_t)nc * maxlat < two16 && 2 * key * key < two32;
  r.keys32 = (uint64_t)nc * a * a < two32 && (uint64_t)nc * maxlat < two16 && 3ull * nc * maxlat < two24 && nc < 256 &&
             (uint64_t)nc * key < two24 && 2 * key * key < two32;
  return r;
}

static void check_fast_limits() {
  // the shipped shapes, nc = R.  Maximum latencies read off the planets:
  // fantoch_amd.planet.Planet.synthetic(64).lat.max() = 350,
  // Planet.synthetic(128).lat.max() = 351, Planet.new().lat.max() = 381 (GCP)
  {
    std::vector<uint16_t> lat(64 * 64, 5);
    lat[17 * 64 + 3] = 350;  // (the maximum is taken over the whole matrix)
    const FastLimits l = fast_limits(lat.data(), 64, 64, 7);
    CHECK(l.maxlat == 350 && l.s32 && l.v32 && l.bins_ok && l.keys32);
    const FastLimits m = fast_limits(350, 64, 7);
    CHECK(m.s2_flush == l.s2_flush && m.g_flush == l.g_flush && m.k_flush == l.k_flush);
  }
  {
    const FastLimits l = fast_limits(351, 128, 6);
    CHECK(l.s32 && l.v32 && l.bins_ok && l.keys32);
  }
  for (uint32_t n : {3u, 5u, 7u, 13u}) {
    const FastLimits l = fast_limits(381, 20, n);
    CHECK(l.s32 && l.v32);
  }
  // v32: max(nc, n) * maxlat = 2^16 - 1 against 2^16, through nc and through n
  CHECK(fast_limits(257, 255, 7).v32 && 255 * 257 == 65535);
  CHECK(!fast_limits(256, 256, 7).v32 && fast_limits(256, 256, 7).s32);
  CHECK(fast_limits(4095, 2, 16).v32 && !fast_limits(4096, 2, 16).v32 && fast_limits(4096, 2, 16).s32);
  // a doubled R=128 planet with 128 clients: 32-bit moments, 64-bit V
  CHECK(fast_limits(600, 128, 6).s32 && !fast_limits(600, 128, 6).v32);
  CHECK(fast_limits(702, 128, 7).s32 && !fast_limits(702, 128, 7).v32);  // 2 * Planet.synthetic(128)
  // s32 at 2^32: max(nc, n) (2 max)^2 = 2^32 at 1024 clients of latency 1024
  CHECK(fast_limits(1024, 1023, 7).s32 && !fast_limits(1024, 1024, 7).s32);
  CHECK(fast_limits(8191, 2, 16).s32 && !fast_limits(8192, 2, 16).s32);  // (n counts: 16 * 16384^2 = 2^32)
  // s32 at 2^24: 3 nc max = 2^24 - 1 (3 * 53261 * 105) against one client more
  CHECK(3ull * 53261 * 105 == (1ull << 24) - 1);
  CHECK(fast_limits(105, 53261, 7).s32 && !fast_limits(105, 53262, 7).s32);
  // bins_ok: the client count, the packed member-pair sums (nc max < 2^16)
  // and two squared keys (2 (16 max + 15)^2 < 2^32: max <= 2895)
  CHECK(fast_limits(200, 255, 7).bins_ok && !fast_limits(200, 256, 7).bins_ok);
  CHECK(fast_limits(257, 255, 7).bins_ok && !fast_limits(258, 255, 7).bins_ok);
  CHECK(fast_limits(2895, 20, 7).bins_ok && !fast_limits(2896, 20, 7).bins_ok);
  CHECK(fast_limits(2895, 20, 7).keys32 && !fast_limits(2896, 20, 7).keys32);
  CHECK(fast_limits(200, 255, 7).keys32 && !fast_limits(200, 256, 7).keys32);
  // keys32's other 2^32 and 2^24 terms (nc (2 max)^2, 3 nc max, nc (16 max +
  // 15)) cannot bind once nc max < 2^16 and max <= 2895 hold, so no input sits
  // on their edges; every term is compared with the restatement instead, on a
  // grid that holds each boundary value and its neighbours
  const uint32_t lats[] = {0, 1, 2, 105, 255, 256, 257, 258, 350, 351, 381, 511, 512, 600, 702, 1023, 1024, 1025,
                           2047, 2048, 2895, 2896, 4095, 4096, 8191, 8192, 16383, 65535};
  const uint32_t ncs[] = {0, 1, 2, 16, 17, 20, 22, 23, 63, 64, 127, 128, 254, 255, 256, 257, 1023, 1024, 4096, 53261,
                          53262};
  for (uint32_t m : lats)
    for (uint32_t nc : ncs)
      for (uint32_t n : {2u, 7u, 16u}) {
        const FastLimits l = fast_limits(m, nc, n);
        const LimitsRef r = limits_ref(m, nc, n);
        CHECK(l.s32 == r.s32 && l.v32 == r.v32 && l.bins_ok == r.bins && l.keys32 == r.keys32);
        CHECK(!l.keys32 || l.bins_ok);
      }
  // flush counts: never 0, and count x the most one quad adds stays inside
  // the accumulator: 4 (2 max)^2 per quad into 32 bits, 2 (2 max) per quad into
  // a packed 16-bit half, 4 (16 max + 15)^2 per quad into 32 bits
  for (uint32_t m : {0u, 1u, 350u, 351u, 381u, 4095u}) {
    const FastLimits l = fast_limits(m, 64, 7);
    const uint64_t amax = 2ull * m, per_quad = 4 * amax * amax, key = 16ull * m + 15, kq = 4 * key * key;
    CHECK(l.s2_flush >= 1 && l.g_flush >= 1 && l.k_flush >= 1);
    CHECK(l.s2_flush <= (1u << 20) && l.g_flush <= l.s2_flush && l.k_flush <= (1u << 20));
    CHECK((uint64_t)l.s2_flush * per_quad < (1ull << 32));
    CHECK((uint64_t)l.g_flush * per_quad < (1ull << 32));
    CHECK((uint64_t)l.g_flush * 2 * amax < (1ull << 16));
    // (one quad of squared keys passes 2^32 from max = 2048 on, where no
    // flush count can help: k_flush is 1 there.  At 4095 the extended keys do
    // not run on the group kernel at all: keys32 is false.)
    if (kq < (1ull << 32)) CHECK((uint64_t)l.k_flush * kq < (1ull << 32));
    else CHECK(l.k_flush == 1);
    if (m == 4095) CHECK(!l.keys32 && !l.bins_ok);
  }
  CHECK(fast_limits(0, 64, 7).s2_flush == (1u << 20) && fast_limits(0, 64, 7).g_flush == (1u << 20));
  CHECK(fast_limits(4095, 64, 7).s2_flush == 16 && fast_limits(4095, 64, 7).g_flush == 4);
}

static void check_score_bands() {
  // bote.py DEFAULT_RANKING: min_mean_fpaxos_improv 110, min_mean_epaxos_improv 35
  for (uint32_t nc : {20u, 64u, 128u}) {
    const ScoreBands b = score_bands(110.0, 35.0, nc);
    CHECK(b.p_int == 1 && b.p1i == 110 * (int64_t)nc && b.p2i == 35 * (int64_t)nc);
    CHECK(b.m1_lo == b.p1i && b.m1_hi == b.p1i && b.m2_lo == b.p2i && b.m2_hi == b.p2i);
  }
  {
    const ScoreBands b = score_bands(-3.0, 0.0, 7);
    CHECK(b.p_int == 1 && b.p1i == -21 && b.p2i == 0 && b.m1_lo == -21 && b.m1_hi == -21 && b.m2_lo == 0);
  }
  // one threshold not an integer: both tests fall back to bands around p * nc
  const double ps[][2] = {{110.5, 35.0}, {110.0, 35.25}, {0.1, -0.1}, {-17.75, 1e-9}, {1234.5678, -999.001}};
  for (auto& p : ps)
    for (uint32_t nc : {1u, 3u, 20u, 64u, 127u, 4096u}) {
      const ScoreBands b = score_bands(p[0], p[1], nc);
      CHECK(b.p_int == 0 && b.p1i == 0 && b.p2i == 0);
      CHECK((double)b.m1_lo <= std::floor(p[0] * nc) - 1 && (double)b.m1_hi >= std::ceil(p[0] * nc) + 1);
      CHECK((double)b.m2_lo <= std::floor(p[1] * nc) - 1 && (double)b.m2_hi >= std::ceil(p[1] * nc) + 1);
      CHECK(b.m1_lo < b.m1_hi && b.m2_lo < b.m2_hi);
    }
  // bands clamp at +-(2^31 - 1), integral or not
  const int32_t cap = 2147483647;
  {
    const ScoreBands b = score_bands(1e9, -1e9, 64);
    CHECK(b.p_int == 1 && b.p1i == 64000000000ll && b.p2i == -64000000000ll);
    CHECK(b.m1_lo == cap && b.m1_hi == cap && b.m2_lo == -cap && b.m2_hi == -cap);
  }
  {
    const ScoreBands b = score_bands(1e9 + 0.5, -1e9 - 0.5, 64);
    CHECK(b.p_int == 0 && b.m1_lo == cap && b.m1_hi == cap && b.m2_lo == -cap && b.m2_hi == -cap);
  }
  {
    const ScoreBands b = score_bands(1e13, 35.0, 2);  // past the integral range: treated as non-integral
    CHECK(b.p_int == 0 && b.m1_hi == cap && b.m2_lo == 69 && b.m2_hi == 71);
  }
}

static void check_objective_sets() {
  // fantoch_amd/bote.py DEFAULT_OBJECTIVES and CONFIG5_OBJECTIVES as (kind, slot)
  const uint32_t def[5][2] = {{0, 0}, {1, 0}, {1, 1}, {2, 0}, {1, 4}};
  const uint32_t c5[8][2] = {{0, 0}, {1, 0}, {1, 1}, {2, 0}, {1, 4}, {1, 10}, {1, 13}, {1, 18}};
  auto match = [](const uint32_t (*o)[2], uint32_t n_obj, uint32_t keys) {
    std::vector<uint32_t> k(n_obj), s(n_obj);
    for (uint32_t i = 0; i < n_obj; ++i) {
      k[i] = o[i][0];
      s[i] = o[i][1];
    }
    return is_compiled_objective_set(k.data(), s.data(), n_obj, keys);
  };
  CHECK(match(def, 5, 0));
  CHECK(match(c5, 8, 1));
  CHECK(!match(def, 5, 1));  // the base set with the extended keys
  CHECK(!match(c5, 8, 0));   // (and the other way round)
  CHECK(!match(c5, 5, 1) && !match(def, 4, 0) && !match(c5, 7, 1) && !match(c5, 6, 0) && !match(def, 0, 0));
  for (uint32_t keys = 0; keys < 2; ++keys) {
    const uint32_t n_obj = keys ? 8 : 5;
    for (uint32_t i = 0; i < n_obj; ++i) {
      uint32_t o[8][2];
      std::memcpy(o, c5, sizeof(o));
      o[i][0] = (o[i][0] + 1) % 3;  // one kind changed
      CHECK(!match(o, n_obj, keys));
      std::memcpy(o, c5, sizeof(o));
      o[i][1] += 1;  // one slot changed: refused, but for SCORE, whose slot is not read
      CHECK(match(o, n_obj, keys) == (i == 0));
    }
  }
  for (uint32_t i = 0; i < COMPILED_OBJECTIVES_KEYS; ++i)
    CHECK(COMPILED_OBJECTIVES[i][0] == c5[i][0] && COMPILED_OBJECTIVES[i][1] == c5[i][1]);
  // slots: f = 2 keys (af2, ff2: 2, 3, 7, 8) need n >= 4; slots 10..19 the extended set
  for (uint32_t n = 2; n <= 16; ++n)
    for (uint32_t slot = 0; slot < 24; ++slot)
      for (uint32_t keys = 0; keys < 2; ++keys) {
        const bool f2 = n >= 4;
        bool want;
        if (slot < 10) want = !(slot % 5 == 2 || slot % 5 == 3) || f2;
        else if (!keys || slot >= 20) want = false;
        else if (slot < 18) want = slot % 2 == 0 || f2;  // tt1, tt2, tw1, tw2 and their colocated four
        else want = slot == 18 || f2;                    // fl1, fl2
        CHECK(slot_exists_n(n, slot, keys) == want);
      }
}

static void check_chunk_states() {
  std::mt19937_64 rng(23);
  const uint32_t shapes[][2] = {{4, 20}, {7, 64}, {16, 20}};
  for (auto& sh : shapes) {
    const uint32_t n = sh[0], ns = sh[1];
    const uint64_t total = binom_u64(ns, n);
    std::vector<uint64_t> starts = {0, total - 1};
    for (int i = 0; i < 500; ++i) starts.push_back(rng() % total);
    std::vector<uint64_t> st;
    CHECK(chunk_states(starts.data(), (uint32_t)starts.size(), n, ns, st));
    CHECK(st.size() == starts.size() * 4);
    std::vector<uint32_t> p(n);
    for (size_t i = 0; i < starts.size(); ++i) {
      CHECK(colex_unrank(starts[i], n, ns, p.data()));
      // word 0: the rank with the three lowest positions' terms zeroed, which
      // is the colex rank of the group's first config (0, 1, 2, p3, ...)
      std::vector<uint32_t> g(p);
      g[0] = 0;
      g[1] = 1;
      g[2] = 2;
      CHECK(st[4 * i] == colex_rank(g.data(), n));
      CHECK(st[4 * i] <= starts[i] && starts[i] - st[4 * i] < binom_u64(p[3], 3));
      // words 1, 2: the n - 3 largest positions, one byte each
      for (uint32_t k = 0; k + 3 < n; ++k) CHECK(((st[4 * i + 1 + k / 8] >> (8 * (k % 8))) & 0xFF) == p[3 + k]);
      for (uint32_t k = n - 3; k < 16; ++k) CHECK(((st[4 * i + 1 + k / 8] >> (8 * (k % 8))) & 0xFF) == 0);
      CHECK(st[4 * i + 3] == 0);
    }
    starts.push_back(total);  // out of range
    CHECK(!chunk_states(starts.data(), (uint32_t)starts.size(), n, ns, st));
  }
  std::vector<uint64_t> st = {1, 2, 3};
  CHECK(chunk_states(nullptr, 0, 7, 64, st) && st.empty());
}

static void check_sample_plan() {
  const uint64_t total = binom_u64(64, 7);
  // a full R=64 n=7 launch on 4,096 waves: 4 one-step chunks per wave
  CHECK(sample_count(0, total, total, 4096, 100) == 16384);
  CHECK(sample_count(0, total, total, 1024, 100) == 4096);
  // shards: steps per wave scale with sqrt(share), rounded up: 1/8 -> 2, 1/64 -> 1
  CHECK(sample_count(0, total / 8, total, 4096, 100) == 8192);
  CHECK(sample_count(total / 2, total / 2 + total / 64, total, 4096, 100) == 4096);
  // at most 4,096 waves' worth of chunks; fewer chunks than K: no seed
  CHECK(sample_count(0, 1ull << 40, 1ull << 40, 1u << 20, 100) == 16384);
  CHECK(sample_count(0, total, total, 16, 100) == 0);
  CHECK(sample_count(0, total, total, 0, 1) == 0);
  // too small to sample: the chunks (64 configs each) may cover at most 1/8 of the range
  CHECK(sample_count(1000, 1000 + 4096ull * 512, total, 4096, 100) == 4096);
  CHECK(sample_count(1000, 1000 + 4096ull * 512 - 1, total, 4096, 100) == 0);
  CHECK(sample_count(0, 0, total, 4096, 100) == 0 && sample_count(0, 63, total, 4096, 1) == 0);
  // a rank space of C(16, 4) = 1,820 never samples, whatever the grid (>= 4 waves: one workgroup) and K
  for (uint32_t nwaves = 4; nwaves <= 8192; ++nwaves)
    for (uint32_t K : {1u, 4u, 128u})
      CHECK(sample_count(0, 1820, 1820, nwaves, K) == 0 && sample_count(97, 97 + 67, 1820, nwaves, K) == 0);
  std::mt19937_64 rng(31);
  for (int i = 0; i < 2000; ++i) {
    const uint64_t tot = i % 2 ? total : binom_u64(128, 6);
    const uint64_t rb = rng() % tot, len = i % 3 ? rng() % (tot - rb + 1) : rng() % std::min<uint64_t>(tot - rb + 1, 1 << 22);
    const uint32_t nwaves = 1 + (uint32_t)(rng() % 8192), K = 1 + (uint32_t)(rng() % 128);
    const uint32_t ns = sample_count(rb, rb + len, tot, nwaves, K);
    if (!ns) continue;
    CHECK(ns >= K && ns <= 65536 && len >= (uint64_t)ns * 512);
    const auto s = sample_starts(rb, rb + len, ns);
    CHECK(s.size() == ns && s.front() == rb && s.back() <= rb + len - 64);
    for (size_t j = 1; j < s.size(); ++j) CHECK(s[j] >= s[j - 1] + 64);
  }
  // runs of consecutive ranks per lane job: ~8 jobs per lane, 1 to 32
  CHECK(sweep_runlen(0, 1024, 256) == 1 && sweep_runlen(1024ull * 256 * 8 * 2 - 1, 1024, 256) == 1);
  CHECK(sweep_runlen(1024ull * 256 * 8 * 2, 1024, 256) == 2);
  CHECK(sweep_runlen(1024ull * 256 * 8 * 32, 1024, 256) == 32 && sweep_runlen(1ull << 62, 1024, 256) == 32);
  for (int i = 0; i < 200; ++i) {
    const uint64_t count = rng() >> (rng() % 50);
    const uint32_t grid = 1 + (uint32_t)(rng() % 4096), bd = 64u << (rng() % 5);
    CHECK(sweep_runlen(count, grid, bd) == std::max<uint64_t>(1, std::min<uint64_t>(32, count / ((uint64_t)grid * bd * 8))));
  }
}

// ------------------------------------------------------ argument checks --
// Every message of the C ABI's argument checks with its code, an accepted
// input next to each boundary, and for the longer entry sequences an input
// that breaks two checks (the earlier one's message must win).
#define REFUSED(expr, want_code, want_msg)                                                              \
  do {                                                                                                  \
    const Status s_ = (expr);                                                                           \
    if (s_.code != (want_code) || s_.msg != (want_msg)) {                                               \
      std::printf("FAIL %s:%d: %s -> %d \"%s\"\n", __FILE__, __LINE__, #expr, s_.code, s_.msg.c_str()); \
      ++failures;                                                                                       \
    }                                                                                                   \
  } while (0)
#define ACCEPTED(expr) REFUSED(expr, BOTE_OK, "")

static void check_arguments() {
  std::vector<uint32_t> ids(4097);  // 0, 1, .., 127, 0, 1, ..: region ids of R = 128
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = (uint32_t)(i % 128);
  const uint32_t* id = ids.data();

  // region lists: R = 1 and 128, ids R - 1 and R, duplicates, null lists
  {
    const uint32_t zero[] = {0}, one[] = {1}, top[] = {5, 127}, over[] = {5, 128}, dup[] = {3, 9, 3};
    ACCEPTED(check_regions(zero, 1, 1, true, "servers"));
    REFUSED(check_regions(one, 1, 1, true, "servers"), BOTE_E_ARG, "servers: region id out of range");
    ACCEPTED(check_regions(top, 2, 128, true, "clients"));
    REFUSED(check_regions(over, 2, 128, false, "clients"), BOTE_E_ARG, "clients: region id out of range");
    ACCEPTED(check_regions(id, 128, 128, true, "servers"));
    REFUSED(check_regions(dup, 3, 128, true, "servers"), BOTE_E_ARG, "servers: duplicate region");
    ACCEPTED(check_regions(dup, 3, 128, false, "froms"));
    ACCEPTED(check_regions(nullptr, 0, 128, true, "froms"));
    REFUSED(check_regions(nullptr, 1, 128, false, "froms"), BOTE_E_ARG, "froms is null");
    CHECK(distinct_count(dup, 3, 128) == 2 && distinct_count(id, 300, 128) == 128 && distinct_count(nullptr, 0, 1) == 0);
  }
  // explicit configs: a position ns, a position twice; the second config is read too
  {
    const uint32_t good[] = {0, 1, 7, 7, 3, 5}, pos_ns[] = {0, 1, 7, 0, 1, 8}, twice[] = {2, 5, 2};
    const uint32_t wide[] = {31, 32, 63, 64, 96, 127};  // every word of the position set
    ACCEPTED(check_configs(good, 2, 3, 8));
    REFUSED(check_configs(pos_ns, 2, 3, 8), BOTE_E_ARG, "config position out of range");
    ACCEPTED(check_configs(pos_ns, 1, 3, 8));
    REFUSED(check_configs(twice, 1, 3, 8), BOTE_E_ARG, "duplicate position in config");
    ACCEPTED(check_configs(wide, 1, 6, 128));
    ACCEPTED(check_configs(nullptr, 0, 3, 8));
  }
  // rank ranges of C(8, 4) = 70 ranks: begin + count and [begin, end] forms
  {
    const char* oob = "rank range out of bounds";
    const struct { uint64_t rb, cnt; bool ok; } ranges[] = {
        {0, 70, true}, {70, 0, true}, {69, 1, true}, {71, 0, false}, {0, 71, false}, {69, 2, false}, {1, ~0ull, false}};
    for (auto& r : ranges) REFUSED(check_rank_range(8, 4, r.rb, r.cnt), r.ok ? BOTE_OK : BOTE_E_ARG, r.ok ? "" : oob);
    const struct { uint64_t rb, re; bool ok; } spans[] = {
        {0, 70, true}, {70, 70, true}, {0, 0, true}, {5, 4, false}, {0, 71, false}, {71, 71, false}};
    for (auto& r : spans) REFUSED(check_rank_span(8, 4, r.rb, r.re), r.ok ? BOTE_OK : BOTE_E_ARG, r.ok ? "" : oob);
  }
  for (int ft = 0; ft <= 3; ++ft)
    REFUSED(check_ft_metric(ft), ft == 1 || ft == 2 ? BOTE_OK : BOTE_E_ARG, ft == 1 || ft == 2 ? "" : "bad ft_metric");

  // search arguments over R = 128: n = 1, 2, 16, 17; n = ns and ns + 1; 4096 and 4097 clients
  {
    const char *small = "config size must be >= 2 (FPaxos q = 2)", *big = "config size above 16",
               *range1 = "config size must be in [1, 16]", *gt = "config size larger than the server list",
               *clients = "more than 4096 clients";
    const struct { uint32_t R, ns, nc, n, min_n; int code; const char* msg; } t[] = {
        {128, 20, 20, 2, 2, BOTE_OK, ""},          {128, 20, 20, 1, 2, BOTE_E_QUORUM_GT_N, small},
        {128, 20, 20, 16, 2, BOTE_OK, ""},         {128, 20, 20, 17, 2, BOTE_E_RANGE, big},
        {128, 20, 20, 1, 1, BOTE_OK, ""},          {128, 20, 20, 0, 1, BOTE_E_RANGE, range1},
        {128, 20, 20, 16, 1, BOTE_OK, ""},         {128, 20, 20, 17, 1, BOTE_E_RANGE, range1},
        {128, 7, 20, 7, 2, BOTE_OK, ""},           {128, 7, 20, 8, 2, BOTE_E_ARG, gt},
        {128, 20, 4096, 5, 2, BOTE_OK, ""},        {128, 20, 4097, 5, 2, BOTE_E_RANGE, clients},
        {0, 20, 20, 5, 2, BOTE_E_ARG, "planet is null"}, {1, 1, 0, 1, 1, BOTE_OK, ""},
        {128, 0, 0, 0, 2, BOTE_E_QUORUM_GT_N, small},  // (the size wins over the empty list)
        {20, 20, 20, 5, 2, BOTE_OK, ""},           {19, 20, 20, 5, 2, BOTE_E_ARG, "servers: region id out of range"},
        {19, 19, 20, 5, 2, BOTE_E_ARG, "clients: region id out of range"}};
    for (auto& c : t) REFUSED(check_search_args(c.R, id, c.ns, id, c.nc, c.n, c.min_n), c.code, c.msg);
    const uint32_t dup[] = {4, 6, 4, 9};
    REFUSED(check_search_args(128, dup, 4, id, 20, 3, 2), BOTE_E_ARG, "servers: duplicate region");
    ACCEPTED(check_search_args(128, id, 20, dup, 4, 3, 2));  // (clients may repeat)
    REFUSED(check_search_args(128, nullptr, 4, id, 20, 3, 2), BOTE_E_ARG, "servers is null");
  }
  // the single-configuration entries (R = 8)
  {
    const uint32_t srv[] = {1, 1, 2}, bad[] = {1, 8, 2};
    const char* gt = "quorum larger than the server set";
    ACCEPTED(check_single_args(8, srv, 3, id, 8, id, 2, 2, 0, 1));  // (2 distinct servers)
    REFUSED(check_single_args(8, srv, 3, id, 8, id, 2, 3, 0, 1), BOTE_E_QUORUM_GT_N, gt);
    REFUSED(check_single_args(8, srv, 3, id, 8, nullptr, 0, 0, 0, 1), BOTE_E_ARG, "quorum size 0");
    REFUSED(check_single_args(8, nullptr, 0, id, 8, nullptr, 0, 1, 0, 1), BOTE_E_QUORUM_GT_N, gt);
    REFUSED(check_single_args(8, bad, 3, id, 8, nullptr, 0, 1, 0, 1), BOTE_E_ARG, "servers: region id out of range");
    REFUSED(check_single_args(8, srv, 3, bad, 3, nullptr, 0, 1, 0, 1), BOTE_E_ARG, "clients: region id out of range");
    REFUSED(check_single_args(8, srv, 3, id, 8, bad, 3, 1, 0, 0), BOTE_E_ARG, "froms: region id out of range");
    REFUSED(check_single_args(8, srv, 3, id, 8, nullptr, 2, 1, 0, 0), BOTE_E_ARG, "froms is null");
    ACCEPTED(check_single_args(8, srv, 3, id, 8, nullptr, 0, 1, 7, 2));
    REFUSED(check_single_args(8, srv, 3, id, 8, nullptr, 0, 1, 8, 2), BOTE_E_ARG, "leader out of range");
    ACCEPTED(check_single_args(8, srv, 3, id, 8, nullptr, 0, 1, 8, 3));  // (only bote_leader reads it)
    // precedence: the lists, the leader, the quorum
    REFUSED(check_single_args(8, bad, 3, bad, 3, nullptr, 0, 0, 8, 2), BOTE_E_ARG, "servers: region id out of range");
    REFUSED(check_single_args(8, srv, 3, id, 8, bad, 3, 0, 8, 2), BOTE_E_ARG, "froms: region id out of range");
    REFUSED(check_single_args(8, srv, 3, id, 8, nullptr, 0, 0, 8, 2), BOTE_E_ARG, "leader out of range");

    const char* none = "the best leader should exist (empty server list)";
    ACCEPTED(check_best_leader_args(8, srv, 3, id, 8, 2, 0));
    ACCEPTED(check_best_leader_args(8, srv, 3, id, 8, 2, 2));
    REFUSED(check_best_leader_args(8, srv, 3, id, 8, 2, 3), BOTE_E_ARG, "unknown stat");
    REFUSED(check_best_leader_args(8, srv, 3, id, 8, 2, -1), BOTE_E_ARG, "unknown stat");
    REFUSED(check_best_leader_args(8, srv, 0, id, 8, 2, 0), BOTE_E_ARG, none);
    REFUSED(check_best_leader_args(8, srv, 3, id, 8, 0, 0), BOTE_E_ARG, "quorum size 0");
    REFUSED(check_best_leader_args(8, srv, 3, id, 8, 3, 0), BOTE_E_QUORUM_GT_N, gt);
    REFUSED(check_best_leader_args(8, srv, 3, bad, 3, 2, 0), BOTE_E_ARG, "clients: region id out of range");
    // precedence: the empty list, the stat, the lists, the quorum
    REFUSED(check_best_leader_args(8, bad, 0, id, 8, 0, 9), BOTE_E_ARG, none);
    REFUSED(check_best_leader_args(8, bad, 3, id, 8, 0, 9), BOTE_E_ARG, "unknown stat");
    REFUSED(check_best_leader_args(8, bad, 3, id, 8, 0, 1), BOTE_E_ARG, "servers: region id out of range");
  }
  // bote_eval / bote_eval_keys and bote_eval_leaderless: 8 servers, n = 4
  {
    bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1F2};
    const uint32_t cfg[] = {0, 1, 2, 7}, pos_ns[] = {0, 1, 2, 8}, twice[] = {0, 1, 1, 7};
    const char *oob = "rank range out of bounds", *ft = "bad ft_metric";
    ACCEPTED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 0, 70, &rp, 0));
    ACCEPTED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 70, 0, nullptr, 1));  // [C, C]
    ACCEPTED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 71, 0, nullptr, 0));  // (no configs: the entry returns first)
    REFUSED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 71, 1, nullptr, 0), BOTE_E_ARG, oob);
    REFUSED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 0, 71, nullptr, 0), BOTE_E_ARG, oob);
    REFUSED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 0, 70, nullptr, 2), BOTE_E_ARG, "unknown key set");
    ACCEPTED(check_eval_args(8, id, 8, id, 8, 4, cfg, 0, 1, &rp, 0));
    REFUSED(check_eval_args(8, id, 8, id, 8, 4, pos_ns, 0, 1, &rp, 0), BOTE_E_ARG, "config position out of range");
    REFUSED(check_eval_args(8, id, 8, id, 8, 4, twice, 0, 1, &rp, 0), BOTE_E_ARG, "duplicate position in config");
    ACCEPTED(check_eval_args(8, id, 8, id, 8, 4, pos_ns, 0, 0, &rp, 0));  // (no configs: nothing is read)
    for (int m : {0, 3}) {
      rp.ft_metric = m;
      REFUSED(check_eval_args(8, id, 8, id, 8, 4, cfg, 0, 1, &rp, 0), BOTE_E_ARG, ft);
      // precedence: key set, planet, sizes, lists, ft_metric, work
      REFUSED(check_eval_args(8, id, 8, id, 8, 4, pos_ns, 0, 1, &rp, 0), BOTE_E_ARG, ft);
      REFUSED(check_eval_args(8, id, 8, id, 8, 4, nullptr, 71, 1, &rp, 0), BOTE_E_ARG, ft);
      REFUSED(check_eval_args(8, id, 8, id, 9, 4, cfg, 0, 1, &rp, 0), BOTE_E_ARG, "clients: region id out of range");
    }
    REFUSED(check_eval_args(0, id, 8, id, 8, 4, cfg, 0, 1, &rp, 2), BOTE_E_ARG, "unknown key set");
    REFUSED(check_eval_args(0, id, 8, id, 8, 1, cfg, 0, 1, &rp, 0), BOTE_E_ARG, "planet is null");
    REFUSED(check_eval_args(8, id, 9, id, 8, 1, cfg, 0, 1, &rp, 0), BOTE_E_QUORUM_GT_N,
            "config size must be >= 2 (FPaxos q = 2)");

    const uint32_t qs[] = {1, 2, 3, 4, 4, 3, 2, 1, 1}, q0[] = {2, 0}, q5[] = {4, 5};
    const char* count = "1 to 8 quorum sizes";
    ACCEPTED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 0, 70, qs, 8));
    ACCEPTED(check_leaderless_args(8, id, 8, id, 8, 1, nullptr, 0, 8, qs, 1));  // n = 1
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 0, nullptr, 0, 1, qs, 1), BOTE_E_RANGE, "config size must be in [1, 16]");
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 0, 70, qs, 9), BOTE_E_ARG, count);
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 0, 70, qs, 0), BOTE_E_ARG, count);
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 0, 70, nullptr, 2), BOTE_E_ARG, count);
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 0, 70, q0, 2), BOTE_E_ARG, "quorum size 0");
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 0, 70, q5, 2), BOTE_E_QUORUM_GT_N, "quorum larger than the config");
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, nullptr, 1, 70, qs, 2), BOTE_E_ARG, oob);
    REFUSED(check_leaderless_args(8, id, 8, id, 8, 4, twice, 0, 1, qs, 2), BOTE_E_ARG, "duplicate position in config");
    ACCEPTED(check_leaderless_args(8, id, 8, id, 8, 4, cfg, 0, 1, qs, 2));
    // precedence: planet, sizes, quorum sizes, lists, work
    REFUSED(check_leaderless_args(0, id, 8, id, 8, 0, cfg, 0, 1, qs, 0), BOTE_E_ARG, "planet is null");
    REFUSED(check_leaderless_args(8, id, 8, id, 4097, 4, cfg, 0, 1, qs, 0), BOTE_E_RANGE, "more than 4096 clients");
    REFUSED(check_leaderless_args(8, id, 9, id, 8, 4, cfg, 0, 1, q5, 2), BOTE_E_QUORUM_GT_N, "quorum larger than the config");
    REFUSED(check_leaderless_args(8, id, 9, id, 8, 4, pos_ns, 0, 1, qs, 2), BOTE_E_ARG, "servers: region id out of range");
  }
  // bote_sweep_create_keys (R = 8 = ns = nc)
  {
    const bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1}, rp0{110.0, 35.0, 0.0, 15.0, 0},
        rp3{110.0, 35.0, 0.0, 15.0, 3};
    std::vector<bote_objective> mean(9, bote_objective{BOTE_OBJ_MEAN, BOTE_SLOT_E});
    bool sc = true;
    auto sweep = [&](uint32_t n, const bote_objective* o, uint32_t n_obj, uint32_t K, const bote_ranking_params* r,
                     int kernel, uint32_t keys, uint32_t R = 8) {
      return check_sweep_args(R, id, 8, id, 8, n, o, n_obj, K, r, kernel, keys, sc);
    };
    const char *kk = "K must be in [1, 128]", *slot = "slot out of range",
               *f2 = "slot does not exist for this n (max_f < 2)", *need = "SCORE objective needs ranking params";
    ACCEPTED(sweep(4, mean.data(), 8, 1, nullptr, BOTE_KERNEL_AUTO, 0));
    CHECK(!sc);
    ACCEPTED(sweep(4, mean.data(), 8, 128, &rp, BOTE_KERNEL_GROUP, 1));
    ACCEPTED(sweep(4, nullptr, 0, 1, nullptr, BOTE_KERNEL_GENERIC, 0));
    REFUSED(sweep(4, mean.data(), 9, 1, nullptr, 0, 0), BOTE_E_RANGE, "more than 8 objectives");
    REFUSED(sweep(4, nullptr, 1, 1, nullptr, 0, 0), BOTE_E_ARG, "objectives null");
    REFUSED(sweep(4, mean.data(), 1, 0, nullptr, 0, 0), BOTE_E_RANGE, kk);
    REFUSED(sweep(4, mean.data(), 1, 129, nullptr, 0, 0), BOTE_E_RANGE, kk);
    REFUSED(sweep(4, mean.data(), 1, 4, nullptr, 0, 2), BOTE_E_ARG, "unknown key set");
    REFUSED(sweep(4, mean.data(), 1, 4, nullptr, -1, 0), BOTE_E_ARG, "unknown kernel path");
    REFUSED(sweep(4, mean.data(), 1, 4, nullptr, 4, 0), BOTE_E_ARG, "unknown kernel path");
    REFUSED(sweep(17, mean.data(), 1, 4, nullptr, 0, 0), BOTE_E_RANGE, "config size above 16");
    const struct { uint32_t kind, slot, n, keys; int code; const char* msg; } objs[] = {
        {BOTE_OBJ_COV, 9, 3, 0, BOTE_OK, ""},     {BOTE_OBJ_COV, 10, 3, 0, BOTE_E_ARG, slot},
        {BOTE_OBJ_MEAN, 19, 4, 1, BOTE_OK, ""},   {BOTE_OBJ_MEAN, 20, 4, 1, BOTE_E_ARG, slot},
        {BOTE_OBJ_MEAN, 10, 4, 1, BOTE_OK, ""},   {BOTE_OBJ_MEAN, BOTE_SLOT_AF2, 4, 0, BOTE_OK, ""},
        {BOTE_OBJ_MEAN, BOTE_SLOT_AF2, 3, 0, BOTE_E_ARG, f2}, {BOTE_OBJ_MEAN, 19, 3, 1, BOTE_E_ARG, f2},
        {3, 0, 4, 0, BOTE_E_ARG, "unknown objective kind"},  {BOTE_OBJ_SCORE, 99, 4, 0, BOTE_E_ARG, need}};
    for (auto& c : objs) {
      const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {c.kind, c.slot}};
      REFUSED(sweep(c.n, o, 2, 4, nullptr, 0, c.keys), c.code, c.msg);
    }
    const bote_objective score[2] = {{BOTE_OBJ_SCORE, 99}, {BOTE_OBJ_MEAN, 10}};  // (a SCORE slot is not read)
    ACCEPTED(sweep(4, score, 1, 4, &rp, 0, 0));
    CHECK(sc);
    REFUSED(sweep(4, score, 1, 4, &rp0, 0, 0), BOTE_E_ARG, "bad ft_metric");
    REFUSED(sweep(4, mean.data(), 1, 4, &rp3, 0, 0), BOTE_E_ARG, "bad ft_metric");  // (checked without SCORE too)
    // precedence: key set, kernel, planet and lists, objective count, null, K, each objective, SCORE's params, ft_metric
    REFUSED(sweep(4, nullptr, 9, 0, nullptr, 9, 2, 0), BOTE_E_ARG, "unknown key set");
    REFUSED(sweep(4, nullptr, 9, 0, nullptr, 9, 1, 0), BOTE_E_ARG, "unknown kernel path");
    REFUSED(sweep(4, nullptr, 9, 0, nullptr, 0, 0, 0), BOTE_E_ARG, "planet is null");
    REFUSED(sweep(9, nullptr, 9, 0, nullptr, 0, 0), BOTE_E_ARG, "config size larger than the server list");
    REFUSED(sweep(4, nullptr, 9, 0, nullptr, 0, 0), BOTE_E_RANGE, "more than 8 objectives");
    REFUSED(sweep(4, nullptr, 2, 0, nullptr, 0, 0), BOTE_E_ARG, "objectives null");
    REFUSED(sweep(4, score, 2, 0, nullptr, 0, 0), BOTE_E_RANGE, kk);
    REFUSED(sweep(4, score, 2, 4, nullptr, 0, 0), BOTE_E_ARG, slot);
    REFUSED(sweep(4, score, 1, 4, nullptr, 0, 0), BOTE_E_ARG, need);
    REFUSED(sweep(4, score, 2, 4, &rp0, 0, 1), BOTE_E_ARG, "bad ft_metric");
  }
  // bote_evolving_chains' levels: n = 3, 5, ..: the popcount, a bit at ns
  {
    const double x[2] = {0, 0};
    const char* bad = "level mask is not an n-subset of the server list";
    auto chain = [&](uint32_t ns, uint32_t level, uint64_t m0, uint64_t m1, bool arrays = true) {
      uint32_t counts[6] = {0, 0, 0, 0, 0, 0};
      const uint64_t m[2] = {m0, m1};
      const uint64_t* masks[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      const double *sc[6] = {x, x, x, x, x, x}, *mn[6] = {x, x, x, x, x, x};
      counts[level] = 2;
      if (arrays) masks[level] = m;
      return check_chain_levels(ns, counts, masks, sc, mn);
    };
    ACCEPTED(chain(5, 0, 0b00111, 0b11100));
    REFUSED(chain(5, 0, 0b00111, 0b01100), BOTE_E_ARG, bad);   // 2 bits at n = 3
    REFUSED(chain(5, 0, 0b00111, 0b11110), BOTE_E_ARG, bad);   // 4 bits
    REFUSED(chain(5, 0, 0b100011, 0b00111), BOTE_E_ARG, bad);  // 3 bits, one at position ns
    ACCEPTED(chain(6, 0, 0b100011, 0b00111));
    ACCEPTED(chain(5, 1, 0b11111, 0b11111));
    REFUSED(chain(5, 1, 0b00111, 0b11111), BOTE_E_ARG, bad);  // n = 5 at level 1
    ACCEPTED(chain(64, 0, 7ull << 61, 0b111));  // (ns = 64: no position is past the mask)
    REFUSED(chain(63, 0, 7ull << 61, 0b111), BOTE_E_ARG, bad);
    REFUSED(chain(5, 2, 0, 0, false), BOTE_E_ARG, "null level array");
    uint32_t none[6] = {0, 0, 0, 0, 0, 0};
    const uint64_t* nomask[6] = {};
    const double* nod[6] = {};
    ACCEPTED(check_chain_levels(5, none, nomask, nod, nod));  // (empty levels need no arrays)
  }
}

int main() {
  check_arguments();
  check_fast_limits();
  check_score_bands();
  check_objective_sets();
  check_chunk_states();
  check_sample_plan();
  check_chunks_per_wave();
  check_geometry();
  check_binomials();
  check_unrank();
  check_walk();
  check_layouts();
  check_unpack();
  if (failures) {
    std::printf("%d host checks failed\n", failures);
    return 1;
  }
  std::printf("host ok\n");
  return 0;
}
