// host_check_evolve.cpp — bounded batches in the host code (bote_host.cpp), run
// under ASan + UBSan by tests/test_evolve_host.py: the limit of
// Search::min_mean_decrease (mean_decrease_limit) against the plain f64
// predicate in a window around the limit and at the ends of the sums' range,
// its monotonicity in both arguments, a set's two limits by ft_metric and n
// (batch_limits), and the new refusals by code, text and order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../fantoch_amd/csrc/bote_host.hpp"

using namespace bote::host;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void refused(const Status& s, int code, const char* text) {
  CHECK(s.code == code);
  if (s.msg != text) {
    std::printf("FAIL text: got \"%s\", want \"%s\"\n", s.msg.c_str(), text);
    ++failures;
  }
}

// Histogram::mean_improv(prev, this) >= min_mean_decrease, as the reference writes it
static bool plain(uint64_t prev_s1, uint64_t s1, uint32_t count, double d) {
  const double prev_mean = (double)prev_s1 / (double)count;
  const double mean = (double)s1 / (double)count;
  return prev_mean - mean >= d;
}

static const uint32_t COUNTS[] = {2, 13, 20, 64, 127, 4096};
static const double DECS[] = {0.0, 15.0, 5.0, 0.1, -3.0, 1e9};
constexpr uint64_t END = 1ull << 27;
constexpr uint64_t WINDOW = 300;

static void check_limit(uint64_t prev, uint32_t c, double d) {
  const uint32_t lim = mean_decrease_limit(prev, c, d);
  CHECK(lim <= END);
  const uint64_t lo = lim > WINDOW ? lim - WINDOW : 0, hi = std::min<uint64_t>(END, (uint64_t)lim + WINDOW);
  for (uint64_t s = lo; s < hi; ++s) {
    const bool want = plain(prev, s, c, d);
    if (want != (s < lim) || want != mean_decrease_passes(prev, s, c, d)) {
      std::printf("FAIL prev %llu count %u dec %g: s1 %llu passes %d, limit %u\n", (unsigned long long)prev, c, d,
                  (unsigned long long)s, (int)want, lim);
      ++failures;
      return;
    }
  }
  CHECK(plain(prev, 0, c, d) == (0 < lim));
  CHECK(plain(prev, END - 1, c, d) == (END - 1 < lim));
}

static void check_limits() {
  for (uint32_t c : COUNTS) {
    // sums of c values of at most 2 * 16383, a few shapes: small, odd, the largest, the range's end
    const uint64_t top = (uint64_t)c * 2 * 16383;
    const uint64_t prevs[] = {0, 1, (uint64_t)c, (uint64_t)c * 15 - 1, (uint64_t)c * 15, (uint64_t)c * 15 + 1,
                              (uint64_t)c * 257 + 3, 1234567 % (top + 1), top / 3, top - 1, top, END - 1};
    for (double d : DECS) {
      uint32_t last = 0;
      bool first = true;
      for (uint64_t prev : prevs) check_limit(prev, c, d);
      // non-decreasing in prev_s1 (a sorted walk)
      for (uint64_t prev = 0; prev < END; prev += END / 97 + 1) {
        const uint32_t lim = mean_decrease_limit(prev, c, d);
        CHECK(first || lim >= last);
        last = lim;
        first = false;
      }
    }
    // non-increasing in min_mean_decrease
    const double asc[] = {-1e9, -3.0, 0.0, 0.1, 5.0, 15.0, 1e9};
    for (uint64_t prev : {(uint64_t)c * 300, top, END - 1}) {
      uint32_t last = (uint32_t)END;
      for (double d : asc) {
        const uint32_t lim = mean_decrease_limit(prev, c, d);
        CHECK(lim <= last);
        last = lim;
      }
    }
  }
  // the ends: nothing passes, everything passes, a threshold that compares false
  CHECK(mean_decrease_limit(0, 20, 15.0) == 0);
  CHECK(mean_decrease_limit(5000, 20, 1e9) == 0);
  CHECK(mean_decrease_limit(0, 20, -1e9) == END);
  CHECK(mean_decrease_limit(5000, 20, -std::numeric_limits<double>::infinity()) == END);
  CHECK(mean_decrease_limit(5000, 20, std::numeric_limits<double>::quiet_NaN()) == 0);
  CHECK(mean_decrease_limit(6000, 20, 0.0) == 6001);  // equal means pass
  CHECK(mean_decrease_limit(6000, 20, 15.0) == 5701);  // 300 - 285 = 15
}

static void check_batch_limits() {
  const uint64_t prev[2] = {6000, 8000};
  uint32_t lim[2];
  // n = 5 over n - 2 = 3: fs(3) = {1} whatever the metric
  batch_limits(prev, 5, 20, 15.0, BOTE_FT_F1F2, lim);
  CHECK(lim[0] == 5701 && lim[1] == MEAN_NO_BOUND);
  // n = 7 over 5: fs(5) = {1, 2} with F1F2, {1} with F1
  batch_limits(prev, 7, 20, 15.0, BOTE_FT_F1F2, lim);
  CHECK(lim[0] == 5701 && lim[1] == 7701);
  batch_limits(prev, 7, 20, 15.0, BOTE_FT_F1, lim);
  CHECK(lim[0] == 5701 && lim[1] == MEAN_NO_BOUND);
  // n = 6 over 4: fs(4) = {1, 2}; n = 3 over 1 and n = 2 over 0: fs is empty
  batch_limits(prev, 6, 20, 0.0, BOTE_FT_F1F2, lim);
  CHECK(lim[0] == 6001 && lim[1] == 8001);
  batch_limits(prev, 3, 20, 15.0, BOTE_FT_F1F2, lim);
  CHECK(lim[0] == MEAN_NO_BOUND && lim[1] == MEAN_NO_BOUND);
  batch_limits(prev, 2, 20, 15.0, BOTE_FT_F1F2, lim);
  CHECK(lim[0] == MEAN_NO_BOUND && lim[1] == MEAN_NO_BOUND);
}

static void check_refusals() {
  uint32_t out = 0;
  // bote_mean_decrease_limit: the null output first, then the count, then the sum
  refused(check_mean_limit_args(END, 0, nullptr), BOTE_E_ARG, "out_limit is null");
  refused(check_mean_limit_args(END, 0, &out), BOTE_E_ARG, "a mean needs count >= 1");
  refused(check_mean_limit_args(END, 20, &out), BOTE_E_RANGE, "previous sum must be below 2^27");
  CHECK(check_mean_limit_args(END - 1, 1, &out).code == BOTE_OK);
  // bote_batch_create_bounded: null params, a null list, no clients, then the sets in order
  bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1F2};
  const uint64_t good[6] = {6000, 8000, 0, 0, END - 1, END - 1};
  const uint64_t bad[6] = {6000, 8000, 5, END, END, 7};
  refused(check_bounded_args(nullptr, 3, 0, nullptr), BOTE_E_ARG, "a bounded batch needs ranking params");
  refused(check_bounded_args(nullptr, 3, 0, &rp), BOTE_E_ARG, "prev_s1 is null");
  refused(check_bounded_args(bad, 3, 0, &rp), BOTE_E_ARG, "a bounded batch needs clients");
  refused(check_bounded_args(bad, 3, 20, &rp), BOTE_E_RANGE, "pinned set 1: previous sum must be below 2^27");
  refused(check_bounded_args(bad + 4, 1, 20, &rp), BOTE_E_RANGE, "pinned set 0: previous sum must be below 2^27");
  CHECK(check_bounded_args(good, 3, 20, &rp).code == BOTE_OK);
  CHECK(check_bounded_args(bad, 1, 20, &rp).code == BOTE_OK);
}

int main() {
  check_limits();
  check_batch_limits();
  check_refusals();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("evolve host ok\n");
  return 0;
}
