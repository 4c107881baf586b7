// bote_host.cpp — host-only pieces of libbote_hip.so (see bote_host.hpp).
// Plain C++ (g++), no HIP: sanitizer builds run it on any CPU.
#include "bote_host.hpp"

#include <algorithm>
#include <cmath>

namespace bote {
namespace host {

uint64_t binom_u64(uint32_t m, uint32_t k) {
  if (k > m) return 0;
  k = std::min(k, m - k);
  unsigned __int128 r = 1;
  for (uint32_t i = 1; i <= k; ++i) {
    r = r * (m - k + i) / i;
    if (r > (unsigned __int128)UINT64_MAX) return 0;
  }
  return (uint64_t)r;
}

std::vector<uint64_t> binom_table(uint32_t ns, uint32_t n) {
  // Pascal's rule, saturating at 0 (= overflow, as binom_u64) from the first
  // overflowing entry of a row on
  std::vector<uint64_t> t((size_t)(ns + 1) * (n + 1), 0);
  for (uint32_t m = 0; m <= ns; ++m) {
    t[(size_t)m * (n + 1)] = 1;
    for (uint32_t k = 1; k <= n && k <= m; ++k) {
      const uint64_t a = t[(size_t)(m - 1) * (n + 1) + k - 1];
      const uint64_t b = k <= m - 1 ? t[(size_t)(m - 1) * (n + 1) + k] : 0;
      const bool ovf = (a == 0) || (k <= m - 1 && b == 0) || b > UINT64_MAX - a;
      t[(size_t)m * (n + 1) + k] = ovf ? 0 : a + b;
    }
  }
  return t;
}

bool colex_unrank(uint64_t rank, uint32_t n, uint32_t ns, uint32_t* out) {
  if (n > ns) return false;
  const uint64_t total = binom_u64(ns, n);
  if (rank >= total) return false;
  uint64_t r = rank;
  uint32_t hi = ns;
  for (int j = (int)n - 1; j >= 0; --j) {
    const uint32_t k = (uint32_t)j + 1;
    uint32_t x = hi - 1;
    while (x > (uint32_t)j && binom_u64(x, k) > r) --x;
    out[j] = x;
    r -= binom_u64(x, k);
    hi = x;
  }
  return true;
}

uint64_t colex_rank(const uint32_t* pos, uint32_t n) {
  uint64_t r = 0;
  for (uint32_t j = 0; j < n; ++j) r += binom_u64(pos[j], j + 1);
  return r;
}

uint64_t pinned_total(uint32_t ns, uint32_t n, uint32_t m) {
  if (m == 0 || m >= n || n > ns) return 0;
  return binom_u64(ns - m, n - m);
}

bool pinned_config(uint64_t pinned_rank, uint32_t n, uint32_t ns, const uint32_t* pinned, uint32_t m, uint32_t* out,
                   uint64_t* out_rank) {
  if (!pinned || !out || m == 0 || m >= n || n > ns) return false;
  std::vector<uint8_t> is_pinned(ns, 0);
  for (uint32_t i = 0; i < m; ++i) {
    if (pinned[i] >= ns || is_pinned[pinned[i]]) return false;
    is_pinned[pinned[i]] = 1;
  }
  std::vector<uint32_t> free_pos;
  for (uint32_t x = 0; x < ns; ++x)
    if (!is_pinned[x]) free_pos.push_back(x);
  const uint32_t F = n - m;
  std::vector<uint32_t> q(F);
  if (!colex_unrank(pinned_rank, F, ns - m, q.data())) return false;
  for (uint32_t i = 0; i < F; ++i) is_pinned[free_pos[q[i]]] = 1;  // (now: is a member)
  uint32_t j = 0;
  for (uint32_t x = 0; x < ns; ++x)
    if (is_pinned[x]) out[j++] = x;
  if (out_rank) *out_rank = colex_rank(out, n);
  return true;
}

// Fitted per-group precompute, in wavefront steps: least squares over the
// per-shard kernel times of scripts/shard_balance.py (profiles/r02h_*): 0.64
// at 64 clients (n=7), 3.7 at 128 clients (n=6); a power of the client count
// in between, clamped outside.
#ifndef BOTE_GROUP_COST
#define BOTE_GROUP_COST 0.0  // 0: fitted per client count
#endif
double group_cost(uint32_t nc) {
  if (BOTE_GROUP_COST > 0) return BOTE_GROUP_COST;
  const double c = 0.64 * std::pow((double)nc / 64.0, 2.53);
  return std::min(8.0, std::max(0.25, c));
}

uint32_t chunks_per_wave(uint64_t ranks, uint32_t nwaves, uint32_t nc, uint32_t cap) {
  const uint32_t lo = std::min<uint32_t>(4, cap);
  if (nwaves == 0) return lo;
  const double T = (double)ranks / 64.0 / (double)nwaves;
  const double c = std::sqrt(T / group_cost(nc));
  return (uint32_t)std::max<double>(lo, std::min<double>(cap, std::floor(c + 0.5)));
}

std::shared_ptr<GroupWalk> walk_groups(uint32_t ns, uint32_t n, uint32_t nc, uint64_t rb, uint64_t re,
                                       uint64_t max_groups) {
  if (re <= rb || n < 4 || n > ns) return nullptr;
  const uint64_t total = binom_u64(ns, n);
  if (total == 0 || re > total) return nullptr;
  const uint32_t F = n - 3;
  const uint64_t all_groups = binom_u64(ns - 3, F);
  // too many groups to walk (each group holds at least one config)
  if ((all_groups == 0 || all_groups > max_groups) && re - rb > max_groups) return nullptr;
  const std::vector<uint64_t> T = binom_table(ns, n);
  auto C = [&](uint32_t m, uint32_t k) { return T[(size_t)m * (n + 1) + k]; };
  std::vector<uint32_t> p(n);
  if (!colex_unrank(rb, n, ns, p.data())) return nullptr;
  std::vector<uint32_t> q(p.begin() + 3, p.end());  // the fixed positions, a combination of {3 .. ns-1}
  auto w = std::make_shared<GroupWalk>();
  w->ns = ns;
  w->n = n;
  w->nc = nc;
  w->rb = rb;
  w->re = re;
  w->group_cost = group_cost(nc);
  const uint64_t expect = std::min<uint64_t>({all_groups ? all_groups : max_groups, re - rb, 1ull << 22});
  w->start.reserve(expect);
  w->len.reserve(expect);
  for (;;) {
    uint64_t base = 0;
    for (uint32_t k = 0; k < F; ++k) base += C(q[k], k + 4);
    const uint64_t g = C(q[0], 3);
    const uint64_t b = std::max(base, rb), e = std::min(base + g, re);
    if (b >= re) break;
    if (e > b) {
      w->start.push_back(b);
      w->len.push_back(e - b);
      if (w->start.size() > max_groups) return nullptr;
    }
    if (e >= re) break;
    // colex successor of the fixed positions
    uint32_t k = 0;
    while (k < F && q[k] + 1 >= (k + 1 < F ? q[k + 1] : ns)) ++k;
    if (k == F) break;
    ++q[k];
    for (uint32_t j = 0; j < k; ++j) q[j] = 3 + j;
  }
  return w;
}

// Boundaries of [b, e) at the given cumulative estimated costs (ascending,
// in wavefront steps; the first chunk starts at b, the last ends at e).
static std::vector<uint64_t> cut_at(const GroupWalk& w, uint64_t b, uint64_t e, const std::vector<double>& targets);

// The total estimated cost of [b, e) (ceil(len / 64) steps + the group cost
// per part of a group), the measure the chunk cuts divide.
static double range_cost(const GroupWalk& w, uint64_t b, uint64_t e) {
  const size_t i0 = (size_t)(std::upper_bound(w.start.begin(), w.start.end(), b) - w.start.begin()) - 1;
  const size_t i1 = (size_t)(std::lower_bound(w.start.begin(), w.start.end(), e) - w.start.begin());
  double total = 0;
  for (size_t i = i0; i < i1; ++i) {
    const uint64_t pb = std::max(w.start[i], b), pl = std::min(w.start[i] + w.len[i], e) - pb;
    total += (double)((pl + 63) / 64) + w.group_cost;
  }
  return total;
}

std::vector<uint64_t> cut_chunks_guided(const GroupWalk& w, uint64_t b, uint64_t e, uint32_t nchunks,
                                        uint32_t tail_waves, uint32_t levels) {
  if (e <= b || nchunks == 0 || !w.covers(b, e) || w.start.empty()) return {};
  // no tail unless the launch has at least 16 base chunks per wave (the tail
  // holds at most 1/16 of the work; on small shards, 8 chunks per wave, the
  // extra chunk-start precomputes cost more than the tail saves: r05q, 1/64
  // of R=64 n=7 0.496 vs 0.481 ms per step)
  if (tail_waves == 0 || levels == 0 || (uint64_t)nchunks < 16ull * tail_waves) return cut_chunks(w, b, e, nchunks);
  const double total = range_cost(w, b, e), c0 = total / nchunks;
  double tail = 0;
  for (uint32_t l = 1; l <= levels; ++l) tail += tail_waves * c0 / (double)(1u << l);
  const double head = total - tail;
  const uint32_t nh = (uint32_t)std::max(1.0, std::floor(head / c0 + 0.5));
  std::vector<double> t;
  t.reserve(nh + (size_t)levels * tail_waves);
  for (uint32_t i = 1; i <= nh; ++i) t.push_back(head * i / nh);
  double at = head;
  for (uint32_t l = 1; l <= levels; ++l)
    for (uint32_t k = 0; k < tail_waves; ++k) {
      at += c0 / (double)(1u << l);
      t.push_back(at);
    }
  t.back() = total;  // (rounding: the last chunk ends at e)
  return cut_at(w, b, e, t);
}

std::vector<uint64_t> cut_chunks(const GroupWalk& w, uint64_t b, uint64_t e, uint32_t nchunks) {
  std::vector<uint64_t> out;
  if (e <= b || nchunks == 0 || !w.covers(b, e) || w.start.empty()) return out;
  // the groups touching [b, e): the walk's clipped groups tile [rb, re)
  const size_t i0 = (size_t)(std::upper_bound(w.start.begin(), w.start.end(), b) - w.start.begin()) - 1;
  const size_t i1 = (size_t)(std::lower_bound(w.start.begin(), w.start.end(), e) - w.start.begin());  // one past
  auto part = [&](size_t i, uint64_t& pb, uint64_t& pl) {
    pb = std::max(w.start[i], b);
    pl = std::min(w.start[i] + w.len[i], e) - pb;
  };
  auto cost = [&](uint64_t pl) { return (double)((pl + 63) / 64) + w.group_cost; };
  double total = 0;
  for (size_t i = i0; i < i1; ++i) {
    uint64_t pb, pl;
    part(i, pb, pl);
    total += cost(pl);
  }
  out.reserve((size_t)nchunks + 1);
  out.push_back(b);
  double cum = 0;
  size_t i = i0;
  for (uint32_t c = 1; c < nchunks; ++c) {
    const double tgt = total * c / nchunks;
    uint64_t pb = 0, pl = 0;
    while (i < i1) {
      part(i, pb, pl);
      if (cum + cost(pl) > tgt) break;
      cum += cost(pl);
      ++i;
    }
    uint64_t bnd = e;
    if (i < i1) bnd = pb + (uint64_t)((tgt - cum) / cost(pl) * (double)pl);
    out.push_back(std::max(out.back(), std::min(bnd, e)));
  }
  out.push_back(e);
  return out;
}

static std::vector<uint64_t> cut_at(const GroupWalk& w, uint64_t b, uint64_t e, const std::vector<double>& targets) {
  std::vector<uint64_t> out;
  const size_t i0 = (size_t)(std::upper_bound(w.start.begin(), w.start.end(), b) - w.start.begin()) - 1;
  const size_t i1 = (size_t)(std::lower_bound(w.start.begin(), w.start.end(), e) - w.start.begin());
  auto part = [&](size_t i, uint64_t& pb, uint64_t& pl) {
    pb = std::max(w.start[i], b);
    pl = std::min(w.start[i] + w.len[i], e) - pb;
  };
  auto cost = [&](uint64_t pl) { return (double)((pl + 63) / 64) + w.group_cost; };
  out.reserve(targets.size() + 1);
  out.push_back(b);
  double cum = 0;
  size_t i = i0;
  for (size_t c = 0; c + 1 < targets.size(); ++c) {
    const double tgt = targets[c];
    uint64_t pb = 0, pl = 0;
    while (i < i1) {
      part(i, pb, pl);
      if (cum + cost(pl) > tgt) break;
      cum += cost(pl);
      ++i;
    }
    uint64_t bnd = e;
    if (i < i1) bnd = pb + (uint64_t)((tgt - cum) / cost(pl) * (double)pl);
    out.push_back(std::max(out.back(), std::min(bnd, e)));
  }
  out.push_back(e);
  return out;
}

// groups with smallest fixed position k hold C(k, 3) configs and run in
// ceil(C(k, 3) / 64) wavefront steps
double group_utilisation(uint32_t ns, uint32_t n) {
  if (n < 4 || n > ns) return 0.0;
  const uint32_t F = n - 3;
  long double cfg = 0, steps = 0;
  for (uint32_t k = 3; k + F <= ns; ++k) {
    const long double groups = (long double)binom_u64(ns - 1 - k, F - 1);
    const uint64_t g = binom_u64(k, 3);
    cfg += groups * g;
    steps += groups * (long double)((g + 63) / 64);
  }
  return steps > 0 ? (double)(cfg / (64 * steps)) : 0.0;
}

bool pick_group_geometry(uint32_t bd, int occ, uint32_t gslots, uint32_t best_bd, int best_occ,
                         uint32_t best_gslots) {
  if (occ <= 0) return false;
  if (best_occ <= 0) return true;
  // client lines for most steps first (up to 8 per wave: a step has 7.7
  // distinct (p1, p2) on average at R=64 n=7, 4.0 at R=128 n=6), then more
  // waves per CU, more client lines, the smaller size.  Measured at R=128
  // n=6: 10 keys 203.4 ms at 256 threads (3 workgroups per
  // CU, 4 lines) vs 183.3 ms at 512 (2 per CU, 16 lines); extended keys
  // 389.2 ms at 256 (no lines) vs 351.5 ms at 512 (1 per CU, 16 lines)
  const uint32_t c = std::min<uint32_t>(gslots, 8), bc = std::min<uint32_t>(best_gslots, 8);
  if (c != bc) return c > bc;
  const uint32_t w = (uint32_t)occ * (bd / 64), bw = (uint32_t)best_occ * (best_bd / 64);
  if (w != bw) return w > bw;
  if (gslots != best_gslots) return gslots > best_gslots;
  return bd < best_bd;
}

uint32_t quad_stride(uint32_t quads) {
  uint32_t s = quads + 1;
  if (s & 1) ++s;
  if ((s / 2) % 2 == 0) s += 2;
  return s;
}

std::vector<uint16_t> quad_layout(const uint16_t* lat, uint32_t R, const uint32_t* rows, uint32_t nrows,
                                  uint32_t shift, uint32_t& quads, uint32_t& stride) {
  quads = (nrows + 3) / 4;
  stride = quad_stride(quads);
  const uint32_t su16 = stride * 4;  // u16 per column
  std::vector<uint16_t> m((size_t)R * su16, 0);
  for (uint32_t t = 0; t < R; ++t)
    for (uint32_t c = 0; c < nrows; ++c) m[(size_t)t * su16 + c] = (uint16_t)(lat[(size_t)rows[c] * R + t] << shift);
  return m;
}

std::vector<uint32_t> low_table(uint32_t m) {
  std::vector<uint32_t> t;
  t.reserve(binom_u64(m, 3));
  for (uint32_t p2 = 2; p2 < m; ++p2)
    for (uint32_t p1 = 1; p1 < p2; ++p1)
      for (uint32_t p0 = 0; p0 < p1; ++p0) t.push_back(p0 | (p1 << 8) | (p2 << 16));
  return t;
}

bool fast_eligible(const uint16_t* lat, uint32_t R, const uint32_t* servers, uint32_t ns, uint32_t nc,
                   bool fairness_threshold) {
  if (nc < 2) return false;
  if (!std::is_sorted(servers, servers + ns)) return false;
  if (fairness_threshold) return false;
  for (size_t i = 0; i < (size_t)R * R; ++i)
    if (lat[i] > 4095) return false;
  for (uint32_t i = 0; i < ns; ++i)
    for (uint32_t j = 0; j < ns; ++j) {
      const uint16_t v = lat[(size_t)servers[i] * R + servers[j]];
      if (i == j ? v != 0 : v == 0) return false;
    }
  return true;
}

// ------------------------------------------------------ sweep planning ---
FastLimits fast_limits(const uint16_t* lat, uint32_t R, uint32_t nc, uint32_t n) {
  uint32_t maxlat = 0;
  for (size_t i = 0; i < (size_t)R * R; ++i) maxlat = std::max<uint32_t>(maxlat, lat[i]);
  return fast_limits(maxlat, nc, n);
}

FastLimits fast_limits(uint32_t maxlat, uint32_t nc, uint32_t n) {
  FastLimits l{};
  l.maxlat = maxlat;
  const uint64_t amax = 2ull * maxlat, per_quad = 4 * amax * amax;
  l.s2_flush = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(1u << 20, per_quad ? 0xFFFFFFFFull / per_quad : 1u << 20));
  // packed-u16 sums (group kernel): each half gains <= 2 * amax per quad
  const uint64_t s1_flush = amax ? 0xFFFFull / (2 * amax) : 1u << 20;
  l.g_flush = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(l.s2_flush, s1_flush));
  // extended keys: squares of the packed keys (latency << 4 | member), two
  // per dot2 into 32 bits (keys32 below requires 2 key^2 < 2^32)
  const uint64_t kmax = 16ull * maxlat + 15, kq = 4 * kmax * kmax;
  l.k_flush = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(1u << 20, 0xFFFFFFFFull / kq));
  // every slot's sum of squares below 2^32 (a value is at most a latency
  // plus a quorum latency, 2 max, over nc >= N clients): the bench-shaped
  // group kernels keep the moments in 32 bits (bote_group.hip S32)
  // (and the FPaxos moments' 24-bit multiplies: column sum + S1 <= 3 nc max < 2^24)
  l.s32 = (uint64_t)std::max(nc, n) * amax * amax < (1ull << 32) && 3ull * nc * maxlat < (1ull << 24);
  // and every V = cnt s2 - s1^2 in 32 bits: V = sum over pairs of
  // (x_i - x_j)^2 <= (cnt / 2)^2 (2 max)^2 = cnt^2 max^2 for values x in
  // [0, 2 max], so cnt max < 2^16 suffices (the kernels compute V mod 2^32
  // from 32-bit products: exact when V < 2^32).  Round 5 asked cnt^2 (2 max)^2
  // < 2^32, which config 5 (128 clients) missed.
  l.v32 = l.s32 && (uint64_t)std::max(nc, n) * maxlat < (1ull << 16);
  // the group kernel's member bins: a client count below 2^8, a sum of nc
  // keys (latency << 4 | member) below 2^24 and two squared keys below 2^32
  // (bote_group.hip)
  l.bins_ok = nc < 256 && (uint64_t)nc * kmax < (1ull << 24) &&
              (uint64_t)nc * maxlat < (1ull << 16) &&  // (packed member-pair bins)
              2 * kmax * kmax < (1ull << 32);
  // the group kernel's extended keys use 32-bit moments: every sum of
  // squares nc * (2 max)^2 and 3 nc max must fit their 32/24 bits
  l.keys32 = l.bins_ok && (uint64_t)nc * amax * amax < (1ull << 32) && 3ull * nc * maxlat < (1ull << 24);
  return l;
}

ScoreBands score_bands(double p_fmean, double p_emean, uint32_t nc) {
  ScoreBands b{};
  auto integral = [](double x) { return x == (double)(int64_t)x && x > -1e12 && x < 1e12; };
  b.p_int = integral(p_fmean) && integral(p_emean) ? 1 : 0;
  b.p1i = b.p_int ? (int64_t)p_fmean * (int64_t)nc : 0;
  b.p2i = b.p_int ? (int64_t)p_emean * (int64_t)nc : 0;
  auto band = [&](double p, int64_t pi, int32_t& lo, int32_t& hi) {
    const double t = p * (double)nc;
    const double l = b.p_int ? (double)pi : std::floor(t) - 1.0, h = b.p_int ? (double)pi : std::ceil(t) + 1.0;
    const double cap = 2147483647.0;  // D = a difference of two sums below 2^21
    lo = (int32_t)std::max(-cap, std::min(cap, l));
    hi = (int32_t)std::max(-cap, std::min(cap, h));
  };
  band(p_fmean, b.p1i, b.m1_lo, b.m1_hi);
  band(p_emean, b.p2i, b.m2_lo, b.m2_hi);
  return b;
}

const uint32_t COMPILED_OBJECTIVES[COMPILED_OBJECTIVES_KEYS][2] = {
    {BOTE_OBJ_SCORE, 0},           {BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MEAN, BOTE_SLOT_FF1},
    {BOTE_OBJ_COV, BOTE_SLOT_AF1}, {BOTE_OBJ_MEAN, BOTE_SLOT_E},   {BOTE_OBJ_MEAN, BOTE_SLOT_TT1},
    {BOTE_OBJ_MEAN, BOTE_SLOT_TW2}, {BOTE_OBJ_MEAN, BOTE_SLOT_FL1}};

bool is_compiled_objective_set(const uint32_t* kinds, const uint32_t* slots, uint32_t n_obj, uint32_t keys) {
  if (n_obj != (keys ? COMPILED_OBJECTIVES_KEYS : COMPILED_OBJECTIVES_BASE)) return false;
  for (uint32_t o = 0; o < n_obj; ++o) {
    const uint32_t kind = COMPILED_OBJECTIVES[o][0];
    if (kinds[o] != kind || (kind != BOTE_OBJ_SCORE && slots[o] != COMPILED_OBJECTIVES[o][1])) return false;
  }
  return true;
}

bool slot_exists_n(uint32_t n, uint32_t slot, uint32_t keys) {
  const bool f2 = n / 2 >= 2;  // bote_max_f(n) >= 2
  if (slot < 10) {
    const uint32_t b = slot % 5;
    return !((b == BOTE_SLOT_AF2 || b == BOTE_SLOT_FF2) && !f2);
  }
  if (!keys || slot >= BOTE_NSLOTS_X) return false;
  if (slot < 18) return (slot - 10) % 2 == 0 || f2;
  return slot == 18 || f2;
}

uint32_t slot_count(uint32_t slot, uint32_t nc, uint32_t n) {
  const bool colocated = (slot >= 5 && slot < 10) || (slot >= 14 && slot < 18);
  return colocated ? n : nc;
}

bool is_percentile_kind(uint32_t kind) { return (kind >> 16) == 1 && (kind & 0xFFFF) >= 1 && (kind & 0xFFFF) <= 9999; }

bool percentile_index(uint32_t bp, uint32_t count, uint32_t& idx, bool& whole) {
  if (bp < 1 || bp > 9999 || count == 0) return false;
  // (volatile: each step is one rounded f64 operation whatever the flags)
  volatile double p = (double)bp / 10000.0;
  volatile double x = p * (double)count;
  volatile double r = std::round(x);
  volatile double d = x - r;
  idx = (uint32_t)r;
  whole = d == 0.0;
  return true;
}

uint32_t percentile_need(uint32_t bp, uint32_t count) {
  uint32_t idx;
  bool whole;
  if (!percentile_index(bp, count, idx, whole)) return 0;
  return count - std::max(idx, 1u) + 1;
}

uint64_t mdtm_half_deviation(const uint32_t* x, uint32_t c) {
  uint64_t s1 = 0, h = 0;
  for (uint32_t i = 0; i < c; ++i) s1 += x[i];
  for (uint32_t i = 0; i < c; ++i)
    if ((uint64_t)c * x[i] > s1) h += (uint64_t)c * x[i] - s1;
  return h;
}

bool mdtm_key(uint64_t H, uint64_t S1, uint64_t& key) {
  if (S1 >= (1ull << MDTM_SUM_BITS) - 1 || H >= (1ull << (64 - MDTM_SUM_BITS))) return false;
  key = (H << MDTM_SUM_BITS) | S1;
  return true;
}

bool chunk_states(const uint64_t* starts, uint32_t count, uint32_t n, uint32_t ns, std::vector<uint64_t>& out) {
  const uint32_t F = n - 3;
  out.assign((size_t)count * 4, 0);
  std::vector<uint32_t> p(n);
  for (uint32_t i = 0; i < count; ++i) {
    if (!colex_unrank(starts[i], n, ns, p.data())) return false;
    uint64_t base = 0, b[2] = {0, 0};
    for (uint32_t k = 0; k < F; ++k) {
      base += binom_u64(p[3 + k], k + 4);
      b[k / 8] |= (uint64_t)p[3 + k] << (8 * (k % 8));
    }
    out[4 * (size_t)i] = base;
    out[4 * (size_t)i + 1] = b[0];
    out[4 * (size_t)i + 2] = b[1];
  }
  return true;
}

// sample steps per wave on a full range (r03v A/B: 8 vs 1, kernel -1.6 %, 1/8
// shard -5 %; r05g: 4 and 8 give the same R=64 n=7 step, 14.15-14.17 vs
// 14.16-14.25 ms, and 4 halves the sample launch: 0.14 vs 0.18 ms outside the kernel)
constexpr uint32_t SEED_STEPS = 4;
uint32_t sample_count(uint64_t rb, uint64_t re, uint64_t total, uint32_t nwaves, uint32_t K) {
  const uint32_t base = std::min<uint32_t>(4096, nwaves);
  // SEED_STEPS one-step chunks per wave, disjoint and at most 1/8 of the
  // range.  (Chunks of 8 consecutive steps, 4,096 of them, measured slower:
  // kernel 15.52 vs 15.35 ms, their K least minima are a looser bound, r03x.)
  const uint64_t fit = (re - rb) / (64 * 8);
  // sample steps per wave: SEED_STEPS on a full sweep; a shard's launch
  // scales them by sqrt(its share of the rank space), rounded up: the sample
  // costs ~ steps, the block merges it saves
  // ~ range / steps, so the best count grows as sqrt(range).  r05g, R=64 n=7
  // shards, 8 scaled (8 / 3 / 1 steps) against 8 fixed: 1/8 shard 2.089 vs
  // 2.125 ms per step, 1/64 0.492 vs 0.531 ms
  const double share = (double)(re - rb) / (double)total;
  const uint32_t steps =
      (uint32_t)std::max(1.0, std::min((double)SEED_STEPS, std::ceil(SEED_STEPS * std::sqrt(share) - 1e-9)));
  const uint32_t nsamp =
      (uint32_t)std::min<uint64_t>({(uint64_t)base * std::max<uint32_t>(1, steps), std::max<uint64_t>(base, fit), 65536});
  if (nsamp < K || re - rb < (uint64_t)nsamp * 64 * 8) return 0;
  return nsamp;
}

std::vector<uint64_t> sample_starts(uint64_t rb, uint64_t re, uint32_t nsamp) {
  std::vector<uint64_t> s(nsamp);
  for (uint32_t i = 0; i < nsamp; ++i) s[i] = rb + (uint64_t)(((unsigned __int128)(re - rb - 64) * i) / nsamp);
  return s;
}

uint32_t sweep_runlen(uint64_t count, uint32_t grid, uint32_t bd) {
  const uint64_t G = (uint64_t)grid * bd;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(32, count / (G * 8)));
}

void unpack_result(const uint8_t* blk, uint32_t n_obj, uint32_t K, uint32_t kp, TopkRecord* out, uint32_t* out_count,
                   uint64_t* out_valid, uint64_t* out_digest) {
  const TopkRecord* r = (const TopkRecord*)blk;
  for (uint32_t o = 0; o < n_obj; ++o) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < K && i < kp; ++i) {
      const TopkRecord x = r[(size_t)o * kp + i];
      if (x.key == ~0ull && x.rank == ~0ull) break;
      if (out) out[(size_t)o * K + i] = x;
      ++c;
    }
    for (uint32_t i = c; out && i < K; ++i) out[(size_t)o * K + i] = TopkRecord{~0ull, ~0ull};
    if (out_count) out_count[o] = c;
  }
  const uint64_t* cnt = (const uint64_t*)(blk + (size_t)n_obj * kp * 16);
  if (out_valid) *out_valid = cnt[0];
  if (out_digest) *out_digest = cnt[1];
}

// ------------------------------------------------------ argument checks --
static Status fail(int code, std::string msg) { return Status{code, std::move(msg)}; }
static const Status OK{};

Status check_regions(const uint32_t* ids, uint32_t n, uint32_t R, bool distinct, const char* what) {
  if (n && !ids) return fail(BOTE_E_ARG, std::string(what) + " is null");
  std::vector<uint8_t> seen(R, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (ids[i] >= R) return fail(BOTE_E_ARG, std::string(what) + ": region id out of range");
    if (distinct && seen[ids[i]]++) return fail(BOTE_E_ARG, std::string(what) + ": duplicate region");
  }
  return OK;
}

uint32_t distinct_count(const uint32_t* ids, uint32_t n, uint32_t R) {
  std::vector<uint8_t> seen(R, 0);
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (!seen[ids[i]]++) ++c;
  return c;
}

Status check_configs(const uint32_t* configs, uint64_t ncfg, uint32_t n, uint32_t ns) {
  for (uint64_t i = 0; i < ncfg; ++i) {
    uint32_t seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // (ns <= 256: the header's precondition)
    for (uint32_t j = 0; j < n; ++j) {
      uint32_t x = configs[i * n + j];
      if (x >= ns) return fail(BOTE_E_ARG, "config position out of range");
      if (seen[x >> 5] & (1u << (x & 31))) return fail(BOTE_E_ARG, "duplicate position in config");
      seen[x >> 5] |= 1u << (x & 31);
    }
  }
  return OK;
}

Status check_rank_range(uint32_t ns, uint32_t n, uint64_t rank_begin, uint64_t ncfg) {
  const uint64_t total = binom_u64(ns, n);
  if (rank_begin > total || ncfg > total - rank_begin) return fail(BOTE_E_ARG, "rank range out of bounds");
  return OK;
}

Status check_rank_span(uint32_t ns, uint32_t n, uint64_t rank_begin, uint64_t rank_end) {
  if (rank_begin > rank_end || rank_end > binom_u64(ns, n)) return fail(BOTE_E_ARG, "rank range out of bounds");
  return OK;
}

Status check_ft_metric(int ft_metric) {
  if (ft_metric != BOTE_FT_F1 && ft_metric != BOTE_FT_F1F2) return fail(BOTE_E_ARG, "bad ft_metric");
  return OK;
}

// check_search_args in its two halves (bote_eval_leaderless checks its quorum
// sizes between them): the sizes, then the lists
static Status check_sizes(uint32_t R, uint32_t ns, uint32_t nc, uint32_t n, uint32_t min_n) {
  if (R == 0) return fail(BOTE_E_ARG, "planet is null");
  if (min_n < 2) {
    if (n < 1 || n > BOTE_MAX_N) return fail(BOTE_E_RANGE, "config size must be in [1, 16]");
  } else {
    if (n < 2) return fail(BOTE_E_QUORUM_GT_N, "config size must be >= 2 (FPaxos q = 2)");
    if (n > BOTE_MAX_N) return fail(BOTE_E_RANGE, "config size above 16");
  }
  if (n > ns) return fail(BOTE_E_ARG, "config size larger than the server list");
  if (nc > BOTE_MAX_CLIENTS) return fail(BOTE_E_RANGE, "more than 4096 clients");
  return OK;
}
static Status check_lists(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc) {
  if (Status s = check_regions(servers, ns, R, true, "servers"); s.code) return s;
  return check_regions(clients, nc, R, false, "clients");
}
// configs, or the rank range without them
static Status check_work(uint32_t ns, uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg) {
  if (ncfg == 0) return OK;
  return configs ? check_configs(configs, ncfg, n, ns) : check_rank_range(ns, n, rank_begin, ncfg);
}

Status check_search_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                         uint32_t n, uint32_t min_n) {
  if (Status s = check_sizes(R, ns, nc, n, min_n); s.code) return s;
  return check_lists(R, servers, ns, clients, nc);
}

static Status check_quorum(uint32_t q, const uint32_t* servers, uint32_t ns, uint32_t R) {
  if (q == 0) return fail(BOTE_E_ARG, "quorum size 0");
  if (q > distinct_count(servers, ns, R)) return fail(BOTE_E_QUORUM_GT_N, "quorum larger than the server set");
  return OK;
}

Status check_single_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                         const uint32_t* froms, uint32_t nf, uint32_t q, uint32_t leader, int mode) {
  if (Status s = check_regions(servers, ns, R, false, "servers"); s.code) return s;
  if (Status s = check_regions(clients, nc, R, false, "clients"); s.code) return s;
  if (Status s = check_regions(froms, nf, R, false, "froms"); s.code) return s;
  if (mode == 2 && leader >= R) return fail(BOTE_E_ARG, "leader out of range");
  return check_quorum(q, servers, ns, R);
}

Status check_best_leader_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                              uint32_t q, int stat) {
  if (ns == 0) return fail(BOTE_E_ARG, "the best leader should exist (empty server list)");
  if (stat < 0 || stat > 2) return fail(BOTE_E_ARG, "unknown stat");
  if (Status s = check_regions(servers, ns, R, false, "servers"); s.code) return s;
  if (Status s = check_regions(clients, nc, R, false, "clients"); s.code) return s;
  return check_quorum(q, servers, ns, R);
}

Status check_eval_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                       uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg,
                       const bote_ranking_params* rp, uint32_t keys) {
  if (keys > BOTE_KEYS_TEMPO_ALL_LEADERS) return fail(BOTE_E_ARG, "unknown key set");
  if (Status s = check_search_args(R, servers, ns, clients, nc, n, 2); s.code) return s;
  if (rp)
    if (Status s = check_ft_metric(rp->ft_metric); s.code) return s;
  return check_work(ns, n, configs, rank_begin, ncfg);
}

Status check_leaderless_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                             uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg,
                             const uint32_t* quorum_sizes, uint32_t nq) {
  if (Status s = check_sizes(R, ns, nc, n, 1); s.code) return s;
  if (nq == 0 || nq > 8 || !quorum_sizes) return fail(BOTE_E_ARG, "1 to 8 quorum sizes");
  for (uint32_t i = 0; i < nq; ++i) {
    if (quorum_sizes[i] == 0) return fail(BOTE_E_ARG, "quorum size 0");
    if (quorum_sizes[i] > n) return fail(BOTE_E_QUORUM_GT_N, "quorum larger than the config");
  }
  if (Status s = check_lists(R, servers, ns, clients, nc); s.code) return s;
  return check_work(ns, n, configs, rank_begin, ncfg);
}

Status check_sweep_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                        uint32_t n, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                        const bote_ranking_params* rp, int kernel, uint32_t keys, bool& has_score) {
  has_score = false;
  if (keys > BOTE_KEYS_TEMPO_ALL_LEADERS) return fail(BOTE_E_ARG, "unknown key set");
  if (kernel < BOTE_KERNEL_AUTO || kernel > BOTE_KERNEL_GROUP) return fail(BOTE_E_ARG, "unknown kernel path");
  if (Status s = check_search_args(R, servers, ns, clients, nc, n, 2); s.code) return s;
  if (n_obj > BOTE_MAX_OBJECTIVES) return fail(BOTE_E_RANGE, "more than 8 objectives");
  if (n_obj && !objs) return fail(BOTE_E_ARG, "objectives null");
  if (K == 0 || K > BOTE_MAX_K) return fail(BOTE_E_RANGE, "K must be in [1, 128]");
  bool has_max = false, has_pctl = false, has_mdtm = false;
  for (uint32_t o = 0; o < n_obj; ++o) {
    const bool pctl = is_percentile_kind(objs[o].kind);
    if (objs[o].kind > BOTE_OBJ_COV && objs[o].kind != BOTE_OBJ_MAX && objs[o].kind != BOTE_OBJ_MDTM && !pctl)
      return fail(BOTE_E_ARG, "unknown objective kind");
    if (objs[o].kind == BOTE_OBJ_SCORE) {
      has_score = true;
      continue;
    }
    if (objs[o].slot >= (keys ? BOTE_NSLOTS_X : BOTE_NSLOTS)) return fail(BOTE_E_ARG, "slot out of range");
    if (!slot_exists_n(n, objs[o].slot, keys)) return fail(BOTE_E_ARG, "slot does not exist for this n (max_f < 2)");
    has_max = has_max || objs[o].kind == BOTE_OBJ_MAX;
    has_mdtm = has_mdtm || objs[o].kind == BOTE_OBJ_MDTM;
    if (pctl) {
      has_pctl = true;
      if (percentile_need(objs[o].kind & 0xFFFF, slot_count(objs[o].slot, nc, n)) > PCTL_MAX_NEED)
        return fail(BOTE_E_RANGE, "percentile needs more than 8 of the slot's largest values");
    }
  }
  // (after the objectives: a bad kind or slot is reported whatever the path)
  if (has_max && kernel == BOTE_KERNEL_GROUP)
    return fail(BOTE_E_ARG, "the group kernel does not compute MAX objectives (fast or generic kernel)");
  if (has_pctl && kernel == BOTE_KERNEL_GROUP)
    return fail(BOTE_E_ARG, "the group kernel does not compute percentile objectives (fast or generic kernel)");
  if (has_mdtm && kernel == BOTE_KERNEL_GROUP)
    return fail(BOTE_E_ARG, "the group kernel does not compute MDTM objectives (fast or generic kernel)");
  if (has_score && !rp) return fail(BOTE_E_ARG, "SCORE objective needs ranking params");
  if (rp) return check_ft_metric(rp->ft_metric);
  return OK;
}

Status check_constraint_args(uint32_t nc, uint32_t n, const bote_constraint* cons, uint32_t n_con, uint32_t n_obj,
                             int kernel, uint32_t keys) {
  if (n_con && !cons) return fail(BOTE_E_ARG, "constraints null");
  for (uint32_t c = 0; c < n_con; ++c) {
    const bool pctl = is_percentile_kind(cons[c].kind);
    if (cons[c].kind > BOTE_OBJ_COV && cons[c].kind != BOTE_OBJ_MAX && cons[c].kind != BOTE_OBJ_MDTM && !pctl)
      return fail(BOTE_E_ARG, "unknown constraint kind");
    if (cons[c].kind == BOTE_OBJ_SCORE) return fail(BOTE_E_ARG, "SCORE is not a constraint kind");
    if (cons[c].slot >= (keys ? BOTE_NSLOTS_X : BOTE_NSLOTS)) return fail(BOTE_E_ARG, "constraint slot out of range");
    if (!slot_exists_n(n, cons[c].slot, keys))
      return fail(BOTE_E_ARG, "constraint slot does not exist for this n (max_f < 2)");
    if (pctl && percentile_need(cons[c].kind & 0xFFFF, slot_count(cons[c].slot, nc, n)) > PCTL_MAX_NEED)
      return fail(BOTE_E_RANGE, "percentile constraint needs more than 8 of the slot's largest values");
  }
  if ((uint64_t)n_obj + n_con > BOTE_MAX_OBJECTIVES)
    return fail(BOTE_E_RANGE, "more than 8 objectives and constraints");
  if (n_con && keys) return fail(BOTE_E_ARG, "constrained sweeps compute the base key set");
  if (n_con && kernel == BOTE_KERNEL_GROUP)
    return fail(BOTE_E_ARG, "the group kernel does not apply constraints (fast or generic kernel)");
  return OK;
}

TailPlan fast_tail_plan(const uint32_t* dev_kinds, uint32_t n_keys) {
  TailPlan t;
  bool mdtm = false;
  for (uint32_t o = 0; o < n_keys; ++o) {
    if (dev_kinds[o] == BOTE_OBJ_MAX) t.tail = std::max(t.tail, (int)TAIL_MAX);
    if (dev_kinds[o] >= DEV_KIND_PCTL) {
      t.tail = TAIL_LIST;
      t.need = std::max(t.need, dev_kinds[o] & DEV_PCTL_NEED_MASK);
    }
    mdtm = mdtm || dev_kinds[o] == BOTE_OBJ_MDTM;
  }
  t.mixed = mdtm && t.tail != TAIL_PLAIN;
  if (mdtm) t.tail = TAIL_MDTM;
  return t;
}

Status check_pinned_args(uint32_t ns, uint32_t n, const uint32_t* pinned, uint32_t n_pinned, int kernel,
                         uint32_t keys) {
  if (!pinned || n_pinned == 0) return fail(BOTE_E_ARG, "pinned list is null or empty");
  if (n_pinned >= n) return fail(BOTE_E_ARG, "pinned members must be fewer than the config size");
  for (uint32_t i = 0; i < n_pinned; ++i)
    if (pinned[i] >= ns) return fail(BOTE_E_ARG, "pinned position out of range");
  for (uint32_t i = 0; i < n_pinned; ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (pinned[i] == pinned[j]) return fail(BOTE_E_ARG, "duplicate pinned position");
  if (kernel == BOTE_KERNEL_GROUP)
    return fail(BOTE_E_ARG, "the group kernel does not sweep pinned members (fast or generic kernel)");
  if (keys) return fail(BOTE_E_ARG, "pinned sweeps compute the base key set");
  return OK;
}

Status check_batch_args(uint32_t ns, uint32_t n, const uint32_t* pinned, uint32_t n_sets, uint32_t m, uint32_t keys) {
  if (n_sets == 0 || n_sets > BATCH_MAX_SETS)
    return fail(BOTE_E_ARG, "a batch takes 1 to " + std::to_string(BATCH_MAX_SETS) + " pinned sets");
  if (!pinned || m == 0 || m >= n) return fail(BOTE_E_ARG, "pinned sets must hold 1 to n - 1 positions");
  for (uint32_t b = 0; b < n_sets; ++b) {
    const uint32_t* set = pinned + (size_t)b * m;
    for (uint32_t i = 0; i < m; ++i)
      if (set[i] >= ns) return fail(BOTE_E_ARG, "pinned set " + std::to_string(b) + ": position out of range");
    for (uint32_t i = 0; i < m; ++i)
      for (uint32_t j = 0; j < i; ++j)
        if (set[i] == set[j]) return fail(BOTE_E_ARG, "pinned set " + std::to_string(b) + ": duplicate position");
  }
  if (keys) return fail(BOTE_E_ARG, "batched pinned sweeps compute the base key set");
  return OK;
}

BatchPlan batch_plan(uint32_t ns, uint32_t n, uint32_t m, uint32_t n_sets, uint32_t grid_cap) {
  BatchPlan p;
  const uint64_t total = pinned_total(ns, n, m);
  if (!total || !n_sets) return p;
  p.total = total;
  const uint64_t passes = (total + BATCH_PASS - 1) / BATCH_PASS;
  const uint64_t fill = grid_cap ? (grid_cap + (uint64_t)n_sets - 1) / n_sets : BATCH_MAX_SLICES;
  p.slices = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({passes, fill, BATCH_MAX_SLICES}));
  p.slice_len = (total + p.slices - 1) / p.slices;
  for (uint32_t s = 0; s <= p.slices; ++s) p.bounds.push_back(std::min<uint64_t>((uint64_t)s * p.slice_len, total));
  p.units = (uint64_t)n_sets * p.slices;
  p.runlen = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(32, (p.slice_len + BATCH_LANES - 1) / BATCH_LANES));
  return p;
}

bool mean_decrease_passes(uint64_t prev_s1, uint64_t s1, uint32_t count, double min_mean_decrease) {
  // (volatile: each step is one rounded f64 operation whatever the flags)
  volatile double c = (double)count;
  volatile double prev_mean = (double)prev_s1 / c;
  volatile double mean = (double)s1 / c;
  volatile double improv = prev_mean - mean;
  return improv >= min_mean_decrease;
}

uint32_t mean_decrease_limit(uint64_t prev_s1, uint32_t count, double min_mean_decrease) {
  // the passing sums are a prefix of [0, MEAN_SUM_END): its length
  uint64_t lo = 0, hi = MEAN_SUM_END;  // every s1 < lo passes, no s1 in [hi, MEAN_SUM_END) does
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (mean_decrease_passes(prev_s1, mid, count, min_mean_decrease)) lo = mid + 1;
    else hi = mid;
  }
  return (uint32_t)lo;
}

void batch_limits(const uint64_t* prev_s1, uint32_t n, uint32_t nc, double min_mean_decrease, int ft_metric,
                  uint32_t* out_lim) {
  // FTMetric::fs(n - 2): f = 1 .. min((n - 2) / 2, 1 or 2)
  const uint32_t minority = n >= 2 ? (n - 2) / 2 : 0;
  const uint32_t fcap = std::min<uint32_t>(minority, ft_metric == BOTE_FT_F1F2 ? 2 : 1);
  for (uint32_t f = 1; f <= 2; ++f)
    out_lim[f - 1] = f <= fcap ? mean_decrease_limit(prev_s1[f - 1], nc, min_mean_decrease) : MEAN_NO_BOUND;
}

Status check_mean_limit_args(uint64_t prev_s1, uint32_t count, const uint32_t* out_limit) {
  if (!out_limit) return fail(BOTE_E_ARG, "out_limit is null");
  if (count == 0) return fail(BOTE_E_ARG, "a mean needs count >= 1");
  if (prev_s1 >= MEAN_SUM_END) return fail(BOTE_E_RANGE, "previous sum must be below 2^27");
  return OK;
}

Status check_bounded_args(const uint64_t* prev_s1, uint32_t n_sets, uint32_t nc, const bote_ranking_params* rp) {
  if (!rp) return fail(BOTE_E_ARG, "a bounded batch needs ranking params");
  if (!prev_s1) return fail(BOTE_E_ARG, "prev_s1 is null");
  if (nc == 0) return fail(BOTE_E_ARG, "a bounded batch needs clients");
  for (uint32_t b = 0; b < n_sets; ++b)
    for (uint32_t f = 0; f < 2; ++f)
      if (prev_s1[2 * (size_t)b + f] >= MEAN_SUM_END)
        return fail(BOTE_E_RANGE, "pinned set " + std::to_string(b) + ": previous sum must be below 2^27");
  return OK;
}

Status check_rank_span_total(uint64_t total, uint64_t rank_begin, uint64_t rank_end) {
  if (rank_begin > rank_end || rank_end > total) return fail(BOTE_E_ARG, "rank range out of bounds");
  return OK;
}

Status check_census_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                         uint32_t n, const bote_objective* objs, uint32_t n_obj, const bote_ranking_params* rp,
                         int kernel, bool& has_score) {
  has_score = false;
  if (kernel == BOTE_KERNEL_GROUP)
    return fail(BOTE_E_ARG, "the group kernel does not run census sweeps (fast or generic kernel)");
  return check_sweep_args(R, servers, ns, clients, nc, n, objs, n_obj, 1, rp, kernel, 0, has_score);
}

Status census_route(bool eligible, const bote_objective* objs, uint32_t n_obj, int kernel, int& path) {
  bool plain = true;  // SCORE, MEAN and COV objectives only
  for (uint32_t o = 0; o < n_obj; ++o) plain = plain && objs[o].kind <= BOTE_OBJ_COV;
  path = 0;
  if (kernel == BOTE_KERNEL_GENERIC) return OK;
  if (kernel == BOTE_KERNEL_FAST) {
    if (!plain)
      return fail(BOTE_E_ARG, "the fast kernel's census variant computes SCORE, MEAN and COV objectives (generic kernel)");
    if (!eligible) return fail(BOTE_E_ARG, "the fast/group kernel is not eligible for this planet and lists");
  }
  path = plain && eligible ? 1 : 0;
  return OK;
}

Status check_census_launch(const TopkRecord* thr, uint32_t n_obj, uint32_t T, uint32_t ns, uint32_t n,
                           uint64_t rank_begin, uint64_t rank_end) {
  if (T == 0 || T > CENSUS_MAX_THRESHOLDS)
    return fail(BOTE_E_ARG, "a census launch takes 1 to " + std::to_string(CENSUS_MAX_THRESHOLDS) + " thresholds per objective");
  if (n_obj && !thr) return fail(BOTE_E_ARG, "thresholds null");
  for (uint32_t o = 0; o < n_obj; ++o)
    for (uint32_t t = 1; t < T; ++t) {
      const TopkRecord &a = thr[(size_t)o * T + t - 1], &b = thr[(size_t)o * T + t];
      if (b.key < a.key || (b.key == a.key && b.rank < a.rank))
        return fail(BOTE_E_ARG, "objective " + std::to_string(o) + ": thresholds must ascend in (key, rank)");
    }
  return check_rank_span(ns, n, rank_begin, rank_end);
}

Status check_chain_levels(uint32_t ns, const uint32_t* counts, const uint64_t* const* masks,
                          const double* const* scores, const double* const* means) {
  for (int l = 0; l < 6; ++l) {
    const uint32_t n = 3 + 2 * l;
    if (counts[l] && (!masks[l] || !scores[l] || !means[l])) return fail(BOTE_E_ARG, "null level array");
    for (uint32_t i = 0; i < counts[l]; ++i) {
      const uint64_t m = masks[l][i];
      if ((uint32_t)__builtin_popcountll(m) != n || (ns < 64 && (m >> ns)))
        return fail(BOTE_E_ARG, "level mask is not an n-subset of the server list");
    }
  }
  return OK;
}

}  // namespace host
}  // namespace bote
