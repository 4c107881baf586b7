// host_check_pctl.cpp — the percentile objective (BOTE_OBJ_PCTL) in the host
// code (fantoch_amd/csrc/bote_host.cpp): percentile_index / percentile_need
// and the argument checks of bote_sweep_create_keys (check_sweep_args), under
// ASan + UBSan on the CPU: built and run by tests/test_pctl_host.py.  R = 32 =
// ns throughout; the client list is the first nc regions.
#include <cstdio>
#include <cstring>

#include "../../fantoch_amd/csrc/bote_host.hpp"

using namespace bote::host;

static int failures = 0;
static void expect(const Status& s, int code, const char* msg, const char* what, int line) {
  if (s.code == code && (code == BOTE_OK || s.msg == msg)) return;
  std::printf("line %d: %s: got (%d, \"%s\"), want (%d, \"%s\")\n", line, what, s.code, s.msg.c_str(), code, msg);
  ++failures;
}
#define ACCEPTED(call) expect((call), BOTE_OK, "", #call, __LINE__)
#define REFUSED(call, code, msg) expect((call), (code), (msg), #call, __LINE__)
#define CHECK(cond)                                        \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("line %d: %s is false\n", __LINE__, #cond); \
      ++failures;                                          \
    }                                                      \
  } while (0)

int main() {
  uint32_t id[32];
  for (uint32_t i = 0; i < 32; ++i) id[i] = i;
  const bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1F2};
  bool sc = false;
  auto sweep = [&](uint32_t nc, uint32_t n, const bote_objective* o, uint32_t n_obj, const bote_ranking_params* r,
                   int kernel, uint32_t keys) { return check_sweep_args(32, id, 32, id, nc, n, o, n_obj, 100, r, kernel, keys, sc); };
  const char *unknown = "unknown objective kind", *slot = "slot out of range",
             *f2 = "slot does not exist for this n (max_f < 2)", *score = "SCORE objective needs ranking params",
             *deep = "percentile needs more than 8 of the slot's largest values",
             *gmax = "the group kernel does not compute MAX objectives (fast or generic kernel)",
             *gpctl = "the group kernel does not compute percentile objectives (fast or generic kernel)";
  static_assert(BOTE_OBJ_PCTL(9500) == 0x10000u + 9500u, "the percentile objective kind");
  static_assert(BOTE_OBJ_PCTL(1) == 0x10001u && BOTE_OBJ_PCTL(9999) == 0x1270Fu, "its range");

  // ---- the index arithmetic: the issue's table (p, count) -> (idx, whole, need)
  {
    const struct {
      uint32_t bp, c, idx;
      bool whole;
      uint32_t need;
    } rows[] = {{9500, 20, 19, true, 2}, {8500, 20, 17, true, 4}, {8000, 20, 16, true, 5}, {6500, 20, 13, true, 8},
                {9900, 20, 20, false, 1}, {9500, 64, 61, false, 4}, {9900, 64, 63, false, 2}, {9500, 128, 122, false, 7},
                {5000, 5, 3, false, 3}, {7500, 9, 7, false, 3}, {1, 1, 0, false, 1}, {1, 4096, 0, false, 4096},
                {5000, 1, 1, false, 1}, {5000, 2, 1, true, 2}, {9999, 4096, 4096, false, 1}};
    for (const auto& r : rows) {
      uint32_t idx = ~0u;
      bool whole = !r.whole;
      CHECK(percentile_index(r.bp, r.c, idx, whole));
      CHECK(idx == r.idx && whole == r.whole);
      CHECK(percentile_need(r.bp, r.c) == r.need);
    }
    uint32_t idx = 7;
    bool whole = true;
    CHECK(!percentile_index(0, 20, idx, whole) && !percentile_index(10000, 20, idx, whole) &&
          !percentile_index(9500, 0, idx, whole));
    CHECK(percentile_need(0, 20) == 0 && percentile_need(10000, 20) == 0 && percentile_need(9500, 0) == 0);
    CHECK(is_percentile_kind(BOTE_OBJ_PCTL(1)) && is_percentile_kind(BOTE_OBJ_PCTL(9999)));
    CHECK(!is_percentile_kind(0x10000u) && !is_percentile_kind(0x10000u | 10000u) && !is_percentile_kind(0x20000u | 9500u) &&
          !is_percentile_kind(9500u) && !is_percentile_kind(BOTE_OBJ_MAX) && !is_percentile_kind(0xFFFFFFFFu));
    CHECK(slot_count(0, 20, 5) == 20 && slot_count(4, 20, 5) == 20 && slot_count(5, 20, 5) == 5 && slot_count(9, 20, 5) == 5 &&
          slot_count(10, 20, 5) == 20 && slot_count(13, 20, 5) == 20 && slot_count(14, 20, 5) == 5 &&
          slot_count(17, 20, 5) == 5 && slot_count(18, 20, 5) == 20 && slot_count(19, 20, 5) == 20);
  }

  // ---- the accepted range of bp: with 8 clients and n <= 8 no percentile needs more than 8 values
  for (uint32_t bp : {1u, 2u, 5000u, 9500u, 9990u, 9998u, 9999u})
    for (uint32_t keys = 0; keys <= 1; ++keys)
      for (uint32_t n = 2; n <= 8; ++n)
        for (uint32_t s = 0; s < (keys ? BOTE_NSLOTS_X : BOTE_NSLOTS); ++s) {
          const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_PCTL(bp), s}};
          for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) {
            if (slot_exists_n(n, s, keys)) ACCEPTED(sweep(8, n, o, 2, nullptr, kernel, keys));
            else REFUSED(sweep(8, n, o, 2, nullptr, kernel, keys), BOTE_E_ARG, f2);
          }
        }
  {
    const bote_objective o[1] = {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_FF1}};
    ACCEPTED(sweep(20, 4, o, 1, nullptr, BOTE_KERNEL_AUTO, 0));
    CHECK(!sc);  // a percentile objective is not SCORE
  }
  // ---- every kind that was unknown stays unknown
  for (uint32_t kind : {3u, 4u, 15u, 17u, 32u, 0xFFFFFFFFu, 0x10000u, 0x10000u | 10000u, 0x10000u | 0xFFFFu, 0x20000u | 9500u,
                        0x1FFFFu, 0x80010000u | 9500u}) {
    const bote_objective o[2] = {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {kind, BOTE_SLOT_AF1}};
    for (uint32_t keys = 0; keys <= 1; ++keys) REFUSED(sweep(20, 4, o, 2, nullptr, BOTE_KERNEL_AUTO, keys), BOTE_E_ARG, unknown);
  }
  // ---- more than 8 of the largest values: BOTE_E_RANGE, by the slot's own count
  {
    // 20 clients: p65 needs 8 (accepted), p60 needs 9, the median 11
    const bote_objective p65[1] = {{BOTE_OBJ_PCTL(6500), BOTE_SLOT_AF1}}, p60[1] = {{BOTE_OBJ_PCTL(6000), BOTE_SLOT_AF1}},
                         p50[1] = {{BOTE_OBJ_PCTL(5000), BOTE_SLOT_FF1}};
    for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) {
      ACCEPTED(sweep(20, 5, p65, 1, nullptr, kernel, 0));
      REFUSED(sweep(20, 5, p60, 1, nullptr, kernel, 0), BOTE_E_RANGE, deep);
      REFUSED(sweep(20, 5, p50, 1, nullptr, kernel, 0), BOTE_E_RANGE, deep);
    }
    // the colocated slots count the n members: the median of 5 needs 3, and of 16 members 9
    const bote_objective c50[1] = {{BOTE_OBJ_PCTL(5000), 5 + BOTE_SLOT_AF1}}, cf50[1] = {{BOTE_OBJ_PCTL(5000), 5 + BOTE_SLOT_FF2}};
    ACCEPTED(sweep(20, 5, c50, 1, nullptr, 0, 0));
    ACCEPTED(sweep(20, 5, cf50, 1, nullptr, 0, 0));
    ACCEPTED(sweep(20, 15, c50, 1, nullptr, 0, 0));  // round(7.5) = 8: 15 - 8 + 1 = 8
    REFUSED(sweep(20, 16, c50, 1, nullptr, 0, 0), BOTE_E_RANGE, deep);
    REFUSED(sweep(8, 16, cf50, 1, nullptr, 0, 0), BOTE_E_RANGE, deep);  // (8 clients: an Input slot would pass)
    // p1 needs every value: 8 clients pass, 9 do not
    const bote_objective p1[1] = {{BOTE_OBJ_PCTL(1), BOTE_SLOT_E}};
    ACCEPTED(sweep(8, 5, p1, 1, nullptr, 0, 0));
    REFUSED(sweep(9, 5, p1, 1, nullptr, 0, 0), BOTE_E_RANGE, deep);
    // the extended key set: Input (tt1, tw2, fl1, fl2) and colocated (tt1C, tw2C) slots
    for (uint32_t s : {(uint32_t)BOTE_SLOT_TT1, (uint32_t)BOTE_SLOT_TW2, (uint32_t)BOTE_SLOT_FL1, (uint32_t)BOTE_SLOT_FL2}) {
      const bote_objective x65[1] = {{BOTE_OBJ_PCTL(6500), s}}, x50[1] = {{BOTE_OBJ_PCTL(5000), s}};
      ACCEPTED(sweep(20, 5, x65, 1, nullptr, 0, 1));
      REFUSED(sweep(20, 5, x50, 1, nullptr, 0, 1), BOTE_E_RANGE, deep);
      REFUSED(sweep(20, 5, x50, 1, nullptr, 0, 0), BOTE_E_ARG, slot);  // (no such slot on the base set)
    }
    for (uint32_t s : {(uint32_t)BOTE_SLOT_TT1 + BOTE_SLOT_X_COLOCATED, (uint32_t)BOTE_SLOT_TW2 + BOTE_SLOT_X_COLOCATED}) {
      const bote_objective x50[1] = {{BOTE_OBJ_PCTL(5000), s}};
      ACCEPTED(sweep(20, 5, x50, 1, nullptr, 0, 1));
      REFUSED(sweep(20, 16, x50, 1, nullptr, 0, 1), BOTE_E_RANGE, deep);
    }
  }
  // ---- a forced group kernel refuses a percentile, with either key set; without one it is accepted
  {
    const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}};
    REFUSED(sweep(20, 4, o, 2, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gpctl);
    REFUSED(sweep(20, 4, o, 2, &rp, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, gpctl);
    ACCEPTED(sweep(20, 4, o, 1, nullptr, BOTE_KERNEL_GROUP, 0));
    for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) ACCEPTED(sweep(20, 4, o, 2, nullptr, kernel, 0));
  }
  // ---- order: per objective kind, slot range, slot existence, depth; then
  // group + MAX, group + percentile, SCORE's params, ft_metric
  {
    const bote_objective far[1] = {{BOTE_OBJ_PCTL(5000), 10}}, absent[1] = {{BOTE_OBJ_PCTL(5000), BOTE_SLOT_AF2}},
                         both[1] = {{0x10000u, 99}};
    REFUSED(sweep(20, 4, far, 1, nullptr, 0, 0), BOTE_E_ARG, slot);      // the slot range before the depth
    REFUSED(sweep(20, 3, absent, 1, nullptr, 0, 0), BOTE_E_ARG, f2);     // the slot's existence before the depth
    REFUSED(sweep(20, 4, absent, 1, nullptr, 0, 0), BOTE_E_RANGE, deep);
    REFUSED(sweep(20, 4, both, 1, nullptr, 0, 0), BOTE_E_ARG, unknown);  // the kind before the slot
    // objectives are checked in turn: the first one's depth before the second one's kind
    const bote_objective dk[2] = {{BOTE_OBJ_PCTL(5000), BOTE_SLOT_AF1}, {17, 0}}, kd[2] = {{17, 0}, {BOTE_OBJ_PCTL(5000), BOTE_SLOT_AF1}};
    REFUSED(sweep(20, 4, dk, 2, nullptr, 0, 0), BOTE_E_RANGE, deep);
    REFUSED(sweep(20, 4, kd, 2, nullptr, 0, 0), BOTE_E_ARG, unknown);
    // the depth (per objective) before the group refusals (after the loop)
    const bote_objective gd[1] = {{BOTE_OBJ_PCTL(5000), BOTE_SLOT_AF1}};
    REFUSED(sweep(20, 4, gd, 1, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_RANGE, deep);
    // a later objective's bad kind or slot before the group refusal
    const bote_objective gk[2] = {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {17, 0}}, gs[2] = {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {BOTE_OBJ_MEAN, 10}};
    REFUSED(sweep(20, 4, gk, 2, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, unknown);
    REFUSED(sweep(20, 4, gs, 2, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, slot);
    // MAX and a percentile on a forced group kernel: the MAX refusal comes first, in either order
    const bote_objective mp[2] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}, {BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}},
                         pm[2] = {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}};
    REFUSED(sweep(20, 4, mp, 2, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gmax);
    REFUSED(sweep(20, 4, pm, 2, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gmax);
    for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) ACCEPTED(sweep(20, 4, mp, 2, nullptr, kernel, 0));
    // group + percentile before SCORE's params and the ft_metric
    const bote_ranking_params rp0{110.0, 35.0, 0.0, 15.0, 0};
    const bote_objective sp[2] = {{BOTE_OBJ_SCORE, 0}, {BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}};
    REFUSED(sweep(20, 4, sp, 2, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gpctl);
    REFUSED(sweep(20, 4, sp, 2, &rp0, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gpctl);
    REFUSED(sweep(20, 4, sp, 2, nullptr, BOTE_KERNEL_FAST, 0), BOTE_E_ARG, score);
    REFUSED(sweep(20, 4, sp, 2, &rp0, BOTE_KERNEL_FAST, 0), BOTE_E_ARG, "bad ft_metric");
    ACCEPTED(sweep(20, 4, sp, 2, &rp, BOTE_KERNEL_FAST, 0));
    // the checks before the objectives are unchanged
    REFUSED(sweep(20, 4, gd, 1, nullptr, BOTE_KERNEL_GROUP, 2), BOTE_E_ARG, "unknown key set");
    REFUSED(sweep(20, 4, gd, 1, nullptr, 4, 0), BOTE_E_ARG, "unknown kernel path");
    REFUSED(sweep(20, 4, gd, 9, nullptr, 0, 0), BOTE_E_RANGE, "more than 8 objectives");
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("pctl host ok\n");
  return 0;
}
