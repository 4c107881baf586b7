// host_check_census.cpp — census sweeps in the host code (bote_host.cpp), run
// under ASan + UBSan by tests/test_census_host.py: the launch checks (T range,
// a null list, the thresholds' order per objective, the rank span) and the
// creation checks (a forced group kernel, then the sweep's own) by code, text
// and order, and the routing of every (objectives, kernel, eligibility) case.
#include <cstdio>
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

constexpr uint64_t ONES = ~0ull;

static void check_launch() {
  static_assert(CENSUS_MAX_THRESHOLDS == 16, "the header's limit");
  // 20 servers, n = 3: 1,140 ranks
  const TopkRecord asc[6] = {{0, 0}, {5, 7}, {5, 7}, {5, 8}, {6, 0}, {ONES, ONES}};
  CHECK(check_census_launch(asc, 1, 6, 20, 3, 0, 1140).code == BOTE_OK);
  CHECK(check_census_launch(asc, 2, 3, 20, 3, 10, 10).code == BOTE_OK);  // two objectives of three; an empty range
  CHECK(check_census_launch(asc, 6, 1, 20, 3, 0, 1).code == BOTE_OK);    // T = 1: nothing to order
  // any u64 is a key: a NaN pattern, a negative double's, all ones with any rank
  const TopkRecord odd[4] = {{0x7FF8000000000000ull, 0}, {0x8000000000000000ull, 3}, {ONES, 0}, {ONES, ONES}};
  CHECK(check_census_launch(odd, 1, 4, 20, 3, 0, 1140).code == BOTE_OK);
  // the T range first, then the null list, then the order, then the span
  refused(check_census_launch(nullptr, 1, 0, 20, 3, 5, 2000), BOTE_E_ARG,
          "a census launch takes 1 to 16 thresholds per objective");
  refused(check_census_launch(nullptr, 1, 17, 20, 3, 5, 2000), BOTE_E_ARG,
          "a census launch takes 1 to 16 thresholds per objective");
  refused(check_census_launch(nullptr, 1, 16, 20, 3, 5, 2000), BOTE_E_ARG, "thresholds null");
  CHECK(check_census_launch(nullptr, 0, 16, 20, 3, 0, 1140).code == BOTE_OK);  // no objectives: nothing to read
  const TopkRecord by_rank[2] = {{5, 8}, {5, 7}};
  refused(check_census_launch(by_rank, 1, 2, 20, 3, 5, 2000), BOTE_E_ARG,
          "objective 0: thresholds must ascend in (key, rank)");
  const TopkRecord by_key[4] = {{1, 1}, {2, 2}, {9, 0}, {8, ONES}};
  refused(check_census_launch(by_key, 2, 2, 20, 3, 0, 1140), BOTE_E_ARG,
          "objective 1: thresholds must ascend in (key, rank)");
  CHECK(check_census_launch(by_key, 1, 3, 20, 3, 0, 1140).code == BOTE_OK);
  // unsigned: a key with the top bit set is above every key without it
  const TopkRecord sign[2] = {{0x8000000000000000ull, 0}, {0x7FFFFFFFFFFFFFFFull, 0}};
  refused(check_census_launch(sign, 1, 2, 20, 3, 0, 1140), BOTE_E_ARG,
          "objective 0: thresholds must ascend in (key, rank)");
  refused(check_census_launch(asc, 1, 6, 20, 3, 0, 1141), BOTE_E_ARG, "rank range out of bounds");
  refused(check_census_launch(asc, 1, 6, 20, 3, 8, 7), BOTE_E_ARG, "rank range out of bounds");
}

static void check_create() {
  std::vector<uint32_t> ids(20);
  for (uint32_t i = 0; i < 20; ++i) ids[i] = i;
  const bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1F2};
  const bote_objective plain[3] = {{BOTE_OBJ_SCORE, 0}, {BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_COV, BOTE_SLOT_FF1}};
  const bote_objective mixed[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}};
  bool has_score = false;
  CHECK(check_census_args(20, ids.data(), 20, ids.data(), 20, 5, plain, 3, &rp, BOTE_KERNEL_AUTO, has_score).code == BOTE_OK);
  CHECK(has_score);
  CHECK(check_census_args(20, ids.data(), 20, ids.data(), 20, 5, mixed, 2, nullptr, BOTE_KERNEL_FAST, has_score).code == BOTE_OK);
  CHECK(!has_score);
  // a forced group kernel before anything else, then the sweep's own checks
  refused(check_census_args(0, nullptr, 0, nullptr, 0, 5, plain, 3, &rp, BOTE_KERNEL_GROUP, has_score), BOTE_E_ARG,
          "the group kernel does not run census sweeps (fast or generic kernel)");
  refused(check_census_args(0, ids.data(), 20, ids.data(), 20, 5, plain, 3, &rp, BOTE_KERNEL_AUTO, has_score), BOTE_E_ARG,
          "planet is null");
  refused(check_census_args(20, ids.data(), 20, ids.data(), 20, 5, plain, 3, &rp, 7, has_score), BOTE_E_ARG,
          "unknown kernel path");
  refused(check_census_args(20, ids.data(), 20, ids.data(), 20, 5, plain, 3, nullptr, BOTE_KERNEL_AUTO, has_score),
          BOTE_E_ARG, "SCORE objective needs ranking params");
  const bote_objective af2[1] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF2}};
  refused(check_census_args(20, ids.data(), 20, ids.data(), 20, 3, af2, 1, &rp, BOTE_KERNEL_AUTO, has_score), BOTE_E_ARG,
          "slot does not exist for this n (max_f < 2)");
  const bote_objective xslot[1] = {{BOTE_OBJ_MEAN, BOTE_SLOT_TT1}};  // the base key set only
  refused(check_census_args(20, ids.data(), 20, ids.data(), 20, 5, xslot, 1, &rp, BOTE_KERNEL_AUTO, has_score), BOTE_E_ARG,
          "slot out of range");
}

static void check_route() {
  const bote_objective plain[3] = {{BOTE_OBJ_SCORE, 0}, {BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_COV, BOTE_SLOT_FF1}};
  const bote_objective tails[3][2] = {{{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}},
                                      {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {BOTE_OBJ_MEAN, BOTE_SLOT_AF1}},
                                      {{BOTE_OBJ_MDTM, BOTE_SLOT_E}, {BOTE_OBJ_COV, BOTE_SLOT_AF1}}};
  int path = -1;
  // SCORE, MEAN and COV objectives: the fast kernel where the planet is eligible
  CHECK(census_route(true, plain, 3, BOTE_KERNEL_AUTO, path).code == BOTE_OK && path == 1);
  CHECK(census_route(true, plain, 3, BOTE_KERNEL_FAST, path).code == BOTE_OK && path == 1);
  CHECK(census_route(true, plain, 3, BOTE_KERNEL_GENERIC, path).code == BOTE_OK && path == 0);
  CHECK(census_route(false, plain, 3, BOTE_KERNEL_AUTO, path).code == BOTE_OK && path == 0);
  CHECK(census_route(false, plain, 3, BOTE_KERNEL_GENERIC, path).code == BOTE_OK && path == 0);
  refused(census_route(false, plain, 3, BOTE_KERNEL_FAST, path), BOTE_E_ARG,
          "the fast/group kernel is not eligible for this planet and lists");
  CHECK(census_route(true, plain, 0, BOTE_KERNEL_AUTO, path).code == BOTE_OK && path == 1);  // no objectives: the valid count
  // a MAX, percentile or MDTM objective: the generic kernel, and no forced fast kernel
  for (const auto& objs : tails) {
    CHECK(census_route(true, objs, 2, BOTE_KERNEL_AUTO, path).code == BOTE_OK && path == 0);
    CHECK(census_route(false, objs, 2, BOTE_KERNEL_AUTO, path).code == BOTE_OK && path == 0);
    CHECK(census_route(true, objs, 2, BOTE_KERNEL_GENERIC, path).code == BOTE_OK && path == 0);
    for (bool eligible : {true, false})
      refused(census_route(eligible, objs, 2, BOTE_KERNEL_FAST, path), BOTE_E_ARG,
              "the fast kernel's census variant computes SCORE, MEAN and COV objectives (generic kernel)");
  }
}

int main() {
  check_launch();
  check_create();
  check_route();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("census host ok\n");
  return 0;
}
