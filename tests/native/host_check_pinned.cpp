// host_check_pinned.cpp — pinned sweeps in the host code (bote_host.cpp), run
// under ASan + UBSan by tests/test_pinned_host.py: every refusal of
// check_pinned_args by code, text and order, what it accepts, and
// pinned_config checked exhaustively against the definition.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
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
  const uint32_t ok3[3] = {7, 2, 5};
  // 1. null or empty
  refused(check_pinned_args(20, 5, nullptr, 2, BOTE_KERNEL_AUTO, 0), BOTE_E_ARG, "pinned list is null or empty");
  refused(check_pinned_args(20, 5, ok3, 0, BOTE_KERNEL_AUTO, 0), BOTE_E_ARG, "pinned list is null or empty");
  // (order: the null list comes before every later refusal)
  refused(check_pinned_args(20, 2, nullptr, 9, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, "pinned list is null or empty");
  // 2. n_pinned >= n (before the positions are read: these are out of range too)
  const uint32_t far3[3] = {70, 70, 99};
  refused(check_pinned_args(20, 3, far3, 3, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG,
          "pinned members must be fewer than the config size");
  refused(check_pinned_args(20, 2, far3, 3, BOTE_KERNEL_AUTO, 0), BOTE_E_ARG,
          "pinned members must be fewer than the config size");
  // 3. a position >= ns (before a repeat: {20, 20} is both)
  const uint32_t out2[2] = {20, 20};
  refused(check_pinned_args(20, 5, out2, 2, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, "pinned position out of range");
  const uint32_t out_late[3] = {3, 3, 20};
  refused(check_pinned_args(20, 5, out_late, 3, BOTE_KERNEL_AUTO, 0), BOTE_E_ARG, "pinned position out of range");
  // 4. a repeated position (before the kernel)
  const uint32_t dup3[3] = {4, 9, 4};
  refused(check_pinned_args(20, 5, dup3, 3, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, "duplicate pinned position");
  // 5. a forced group kernel (before the key set)
  refused(check_pinned_args(20, 5, ok3, 3, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG,
          "the group kernel does not sweep pinned members (fast or generic kernel)");
  // 6. the extended key set
  refused(check_pinned_args(20, 5, ok3, 3, BOTE_KERNEL_AUTO, BOTE_KEYS_TEMPO_ALL_LEADERS), BOTE_E_ARG,
          "pinned sweeps compute the base key set");
  // accepted: m = 1, m = n - 1, unsorted input, each kernel but the group one
  const uint32_t one[1] = {19};
  CHECK(check_pinned_args(20, 5, one, 1, BOTE_KERNEL_AUTO, 0).code == BOTE_OK);
  const uint32_t four[4] = {19, 0, 7, 3};
  CHECK(check_pinned_args(20, 5, four, 4, BOTE_KERNEL_FAST, 0).code == BOTE_OK);
  CHECK(check_pinned_args(20, 5, ok3, 3, BOTE_KERNEL_GENERIC, 0).code == BOTE_OK);
  CHECK(check_pinned_args(2, 2, one, 1, BOTE_KERNEL_AUTO, 0).code == BOTE_E_ARG);  // 19 >= ns = 2
  // the pinned rank span
  CHECK(check_rank_span_total(816, 0, 816).code == BOTE_OK);
  CHECK(check_rank_span_total(816, 816, 816).code == BOTE_OK);
  refused(check_rank_span_total(816, 0, 817), BOTE_E_ARG, "rank range out of bounds");
  refused(check_rank_span_total(816, 5, 4), BOTE_E_ARG, "rank range out of bounds");
}

static void check_shape(uint32_t ns, uint32_t n, uint32_t m, const std::vector<uint32_t>& pinned) {
  const uint64_t total = pinned_total(ns, n, m);
  CHECK(total == binom_u64(ns - m, n - m) && total > 0);
  std::set<std::vector<uint32_t>> seen;
  uint64_t prev = 0;
  std::vector<uint32_t> pos(n);
  for (uint64_t pr = 0; pr < total; ++pr) {
    uint64_t full = ~0ull;
    CHECK(pinned_config(pr, n, ns, pinned.data(), m, pos.data(), &full));
    for (uint32_t j = 0; j < n; ++j) CHECK(pos[j] < ns && (j == 0 || pos[j - 1] < pos[j]));
    for (uint32_t x : pinned) CHECK(std::find(pos.begin(), pos.end(), x) != pos.end());
    CHECK(full == colex_rank(pos.data(), n));
    CHECK(pr == 0 || full > prev);  // full ranks strictly increase with the pinned rank
    prev = full;
    // the full rank unranks to the same config
    std::vector<uint32_t> back(n);
    CHECK(colex_unrank(full, n, ns, back.data()) && back == pos);
    seen.insert(pos);
  }
  CHECK(seen.size() == total);  // exactly the supersets: C(ns - m, n - m) distinct ones
  uint64_t dummy;
  CHECK(!pinned_config(total, n, ns, pinned.data(), m, pos.data(), &dummy));
  CHECK(pinned_config(0, n, ns, pinned.data(), m, pos.data(), nullptr));  // out_rank may be null
}

static void check_configs() {
  const uint32_t shapes[6][3] = {{9, 4, 1}, {9, 4, 3}, {10, 5, 2}, {8, 3, 2}, {11, 7, 4}, {20, 13, 1}};
  for (const auto& sh : shapes) {
    const uint32_t ns = sh[0], n = sh[1], m = sh[2];
    std::vector<uint32_t> low, high, inter;
    for (uint32_t i = 0; i < m; ++i) {
      low.push_back(i);
      high.push_back(ns - 1 - i);                 // (descending: unsorted input, includes ns - 1)
      inter.push_back((1 + i * (ns - 2) / m) % ns);  // spread over the positions
    }
    std::reverse(inter.begin(), inter.end());
    check_shape(ns, n, m, low);
    check_shape(ns, n, m, high);
    check_shape(ns, n, m, inter);
  }
  // sizes and lists pinned_total / pinned_config refuse
  CHECK(pinned_total(20, 5, 0) == 0 && pinned_total(20, 5, 5) == 0 && pinned_total(4, 5, 1) == 0);
  CHECK(pinned_total(20, 5, 2) == 816 && pinned_total(64, 7, 2) == 6471002 && pinned_total(128, 7, 2) == 244222650);
  uint32_t pos[16];
  const uint32_t dup[2] = {3, 3}, far[2] = {3, 20}, fine[2] = {3, 4};
  CHECK(!pinned_config(0, 5, 20, dup, 2, pos, nullptr));
  CHECK(!pinned_config(0, 5, 20, far, 2, pos, nullptr));
  CHECK(!pinned_config(0, 5, 20, nullptr, 2, pos, nullptr));
  CHECK(!pinned_config(0, 2, 20, fine, 2, pos, nullptr));
  CHECK(pinned_config(815, 5, 20, fine, 2, pos, nullptr) && pos[4] == 19 && pos[0] == 3 && pos[1] == 4);
}

int main() {
  check_args();
  check_configs();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("pinned host ok\n");
  return 0;
}
