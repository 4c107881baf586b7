// host_check_batch.cpp — batched pinned sweeps in the host code (bote_host.cpp),
// run under ASan + UBSan by tests/test_batch_host.py: every refusal of
// check_batch_args by code, text and order, what it accepts, and the unit plan
// (batch_plan) over the shapes of the GPU tests: the units' slices cover each
// set's pinned ranks exactly once, at most 7 slices, B * S units.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

static void check_args() {
  const uint32_t ok[6] = {7, 2, 5, 2, 7, 19};  // two sets of 3 (equal as sets), or three of 2
  // 1. the set count (before everything else: the list is null, m is bad, keys are set)
  refused(check_batch_args(20, 5, nullptr, 0, 9, 1), BOTE_E_ARG, "a batch takes 1 to 1024 pinned sets");
  refused(check_batch_args(20, 5, ok, 1025, 3, 0), BOTE_E_ARG, "a batch takes 1 to 1024 pinned sets");
  // 2. m out of range or a null list (before the positions are read)
  const uint32_t far[4] = {70, 70, 99, 99};
  refused(check_batch_args(20, 5, nullptr, 2, 2, 1), BOTE_E_ARG, "pinned sets must hold 1 to n - 1 positions");
  refused(check_batch_args(20, 5, far, 2, 0, 1), BOTE_E_ARG, "pinned sets must hold 1 to n - 1 positions");
  refused(check_batch_args(20, 2, far, 2, 2, 1), BOTE_E_ARG, "pinned sets must hold 1 to n - 1 positions");
  refused(check_batch_args(20, 5, far, 1, 5, 0), BOTE_E_ARG, "pinned sets must hold 1 to n - 1 positions");
  // 3. a bad set, the lowest index first; within a set a position >= ns before a repeat
  const uint32_t out1[6] = {1, 2, 3, 20, 20, 4};
  refused(check_batch_args(20, 5, out1, 2, 3, 1), BOTE_E_ARG, "pinned set 1: position out of range");
  const uint32_t dup0[6] = {4, 9, 4, 20, 20, 4};
  refused(check_batch_args(20, 5, dup0, 2, 3, 1), BOTE_E_ARG, "pinned set 0: duplicate position");
  const uint32_t dup2[6] = {4, 9, 1, 2, 6, 6};
  refused(check_batch_args(20, 5, dup2, 3, 2, 0), BOTE_E_ARG, "pinned set 2: duplicate position");
  // 4. the extended key set
  refused(check_batch_args(20, 5, ok, 2, 3, BOTE_KEYS_TEMPO_ALL_LEADERS), BOTE_E_ARG,
          "batched pinned sweeps compute the base key set");
  // accepted: equal sets, overlapping sets, unsorted input, m = 1, m = n - 1, 1024 sets
  CHECK(check_batch_args(20, 5, ok, 2, 3, 0).code == BOTE_OK);
  CHECK(check_batch_args(20, 5, ok, 3, 2, 0).code == BOTE_OK);
  CHECK(check_batch_args(20, 5, ok, 6, 1, 0).code == BOTE_OK);
  const uint32_t four[4] = {19, 0, 7, 3};
  CHECK(check_batch_args(20, 5, four, 1, 4, 0).code == BOTE_OK);
  std::vector<uint32_t> many(1024, 3);
  CHECK(check_batch_args(20, 5, many.data(), 1024, 1, 0).code == BOTE_OK);
  // a forced group kernel is the pinned sweep's refusal, on set 0
  refused(check_pinned_args(20, 5, ok, 3, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG,
          "the group kernel does not sweep pinned members (fast or generic kernel)");
}

static void check_plan(uint32_t ns, uint32_t n, uint32_t m, uint32_t B, uint32_t cap, uint32_t want_slices) {
  const BatchPlan p = batch_plan(ns, n, m, B, cap);
  const uint64_t total = pinned_total(ns, n, m);
  CHECK(total > 0 && p.total == total);
  CHECK(p.slices >= 1 && p.slices <= 7 && p.slices == want_slices);
  CHECK(p.units == (uint64_t)B * p.slices);
  CHECK(p.bounds.size() == (size_t)p.slices + 1);
  // the slices cover [0, total) exactly once: consecutive, ascending, none empty
  CHECK(p.bounds.front() == 0 && p.bounds.back() == total);
  for (uint32_t s = 0; s < p.slices; ++s) {
    CHECK(p.bounds[s] < p.bounds[s + 1]);
    // (what the kernel computes for slice s from slice_len and the total)
    const uint64_t rb = std::min<uint64_t>((uint64_t)s * p.slice_len, total);
    CHECK(rb == p.bounds[s] && std::min<uint64_t>(rb + p.slice_len, total) == p.bounds[s + 1]);
  }
  // every unit (set, slice) is one index below the unit count, each once
  std::vector<uint8_t> seen(p.units, 0);
  for (uint32_t b = 0; b < B; ++b)
    for (uint32_t s = 0; s < p.slices; ++s) {
      const uint64_t u = (uint64_t)b * p.slices + s;
      CHECK(u < p.units && !seen[u] && u / p.slices == b && u % p.slices == s);
      seen[u] = 1;
    }
  CHECK(p.runlen >= 1 && p.runlen <= 32);
  // one slice fits the lanes' runs in one pass whenever the set fits one pass
  if (total <= BATCH_PASS) CHECK(p.slices == 1 && (uint64_t)p.runlen * BATCH_LANES >= total);
}

static void check_plans() {
  check_plan(20, 3, 2, 190, 0, 1);   // 18 configs per set
  check_plan(20, 5, 3, 40, 3, 1);    // 136
  check_plan(64, 7, 5, 100, 0, 1);   // 1,711
  check_plan(64, 6, 1, 2, 0, 7);     // 7,028,847: sliced
  check_plan(48, 6, 1, 2, 0, 7);     // 1,533,939
  check_plan(8, 8, 7, 5, 0, 1);      // one config per set (ns = n = m + 1)
  check_plan(64, 6, 1, 2, 1024, 7);  // the grid cap asks for 512 slices per set: capped at 7
  check_plan(64, 6, 1, 400, 1024, 3);  // ... for 3
  check_plan(64, 6, 1, 1024, 1024, 1);
  check_plan(20, 5, 2, 4, 0, 1);     // 816 <= one pass
  check_plan(30, 6, 2, 4, 0, 3);     // 20,475: 3 passes
  // bad sizes: no plan
  CHECK(batch_plan(20, 5, 0, 4, 0).slices == 0 && batch_plan(20, 5, 5, 4, 0).slices == 0);
  CHECK(batch_plan(4, 5, 1, 4, 0).slices == 0 && batch_plan(20, 5, 2, 0, 0).slices == 0);
}

int main() {
  check_args();
  check_plans();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("batch host ok\n");
  return 0;
}
