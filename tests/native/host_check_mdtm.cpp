// host_check_mdtm.cpp — the MDTM objective (BOTE_OBJ_MDTM) in the host code
// (fantoch_amd/csrc/bote_host.cpp): the argument checks of
// bote_sweep_create_keys (check_sweep_args) and the key's bounds, under ASan +
// UBSan on the CPU: built and run by tests/test_mdtm_host.py.  R = 8 = ns = nc
// throughout the argument checks.
#include <cstdio>
#include <cstring>
#include <vector>

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
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s is false\n", __LINE__, #cond);   \
      ++failures;                                               \
    }                                                           \
  } while (0)

int main() {
  const uint32_t id[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  const bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1F2}, rp0{110.0, 35.0, 0.0, 15.0, 0};
  bool sc = false;
  auto sweep = [&](uint32_t n, const bote_objective* o, uint32_t n_obj, uint32_t K, const bote_ranking_params* r,
                   int kernel, uint32_t keys) { return check_sweep_args(8, id, 8, id, 8, n, o, n_obj, K, r, kernel, keys, sc); };
  const char *unknown = "unknown objective kind", *slot = "slot out of range",
             *f2 = "slot does not exist for this n (max_f < 2)", *need = "SCORE objective needs ranking params",
             *gmax = "the group kernel does not compute MAX objectives (fast or generic kernel)",
             *gpctl = "the group kernel does not compute percentile objectives (fast or generic kernel)",
             *gmdtm = "the group kernel does not compute MDTM objectives (fast or generic kernel)";
  static_assert(BOTE_OBJ_MDTM == 18, "the MDTM objective kind");
  static_assert(BOTE_MDTM_SUM_BITS == 27 && MDTM_SUM_BITS == 27, "the key's sum field");

  // kind 18 with every existing slot of either key set, on auto, generic and fast
  for (uint32_t keys = 0; keys <= 1; ++keys)
    for (uint32_t n = 2; n <= 8; ++n)
      for (uint32_t s = 0; s < (keys ? BOTE_NSLOTS_X : BOTE_NSLOTS); ++s) {
        const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MDTM, s}};
        for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) {
          if (slot_exists_n(n, s, keys)) ACCEPTED(sweep(n, o, 2, 100, nullptr, kernel, keys));
          else REFUSED(sweep(n, o, 2, 100, nullptr, kernel, keys), BOTE_E_ARG, f2);  // MDTM on a slot absent for n
        }
      }
  {
    const bote_objective o[1] = {{BOTE_OBJ_MDTM, BOTE_SLOT_FF1}};
    ACCEPTED(sweep(4, o, 1, 1, nullptr, BOTE_KERNEL_AUTO, 0));
    if (sc) {
      std::printf("an MDTM objective reported as SCORE\n");
      ++failures;
    }
  }
  // the neighbouring kinds stay unknown
  for (uint32_t kind : {3u, 4u, 15u, 17u, 19u, 32u}) {
    const bote_objective o[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {kind, BOTE_SLOT_AF1}};
    for (uint32_t keys = 0; keys <= 1; ++keys) REFUSED(sweep(4, o, 2, 4, nullptr, BOTE_KERNEL_AUTO, keys), BOTE_E_ARG, unknown);
  }
  // the slot range and slot existence apply to MDTM as to MEAN
  {
    const bote_objective s10[1] = {{BOTE_OBJ_MDTM, 10}}, s20[1] = {{BOTE_OBJ_MDTM, 20}},
                         a2[1] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF2}}, fl2[1] = {{BOTE_OBJ_MDTM, BOTE_SLOT_FL2}};
    const bote_objective m10[1] = {{BOTE_OBJ_MEAN, 10}}, m20[1] = {{BOTE_OBJ_MEAN, 20}},
                         ma2[1] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF2}}, mfl2[1] = {{BOTE_OBJ_MEAN, BOTE_SLOT_FL2}};
    for (const bote_objective* o : {s10, m10}) {
      REFUSED(sweep(4, o, 1, 4, nullptr, 0, 0), BOTE_E_ARG, slot);
      ACCEPTED(sweep(4, o, 1, 4, nullptr, 0, 1));
    }
    for (const bote_objective* o : {s20, m20}) REFUSED(sweep(4, o, 1, 4, nullptr, 0, 1), BOTE_E_ARG, slot);
    for (const bote_objective* o : {a2, ma2}) {
      REFUSED(sweep(3, o, 1, 4, nullptr, 0, 0), BOTE_E_ARG, f2);
      ACCEPTED(sweep(4, o, 1, 4, nullptr, 0, 0));
    }
    for (const bote_objective* o : {fl2, mfl2}) REFUSED(sweep(3, o, 1, 4, nullptr, 0, 1), BOTE_E_ARG, f2);
  }
  // a forced group kernel refuses MDTM, with either key set; without MDTM it is accepted
  {
    const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MDTM, BOTE_SLOT_AF1}};
    REFUSED(sweep(4, o, 2, 100, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gmdtm);
    REFUSED(sweep(4, o, 2, 100, &rp, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, gmdtm);
    ACCEPTED(sweep(4, o, 1, 100, nullptr, BOTE_KERNEL_GROUP, 0));
  }
  // ... after the MAX and percentile refusals when those kinds are present too, in any order
  {
    const bote_objective dm[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}},
                         md[2] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}, {BOTE_OBJ_MDTM, BOTE_SLOT_AF1}},
                         dp[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}},
                         pd[2] = {{BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {BOTE_OBJ_MDTM, BOTE_SLOT_AF1}},
                         all[3] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {BOTE_OBJ_PCTL(9500), BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}};
    for (uint32_t keys = 0; keys <= 1; ++keys) {
      REFUSED(sweep(4, dm, 2, 4, nullptr, BOTE_KERNEL_GROUP, keys), BOTE_E_ARG, gmax);
      REFUSED(sweep(4, md, 2, 4, nullptr, BOTE_KERNEL_GROUP, keys), BOTE_E_ARG, gmax);
      REFUSED(sweep(4, dp, 2, 4, nullptr, BOTE_KERNEL_GROUP, keys), BOTE_E_ARG, gpctl);
      REFUSED(sweep(4, pd, 2, 4, nullptr, BOTE_KERNEL_GROUP, keys), BOTE_E_ARG, gpctl);
      REFUSED(sweep(4, all, 3, 4, nullptr, BOTE_KERNEL_GROUP, keys), BOTE_E_ARG, gmax);
    }
    // off the group kernel the mixed sweeps pass the argument checks (the planner routes them)
    for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) {
      ACCEPTED(sweep(4, dm, 2, 4, nullptr, kernel, 0));
      ACCEPTED(sweep(4, all, 3, 4, nullptr, kernel, 0));
    }
  }
  // order: a later objective's bad kind, slot or absent slot comes before the
  // group refusal; the group refusal before SCORE's params and the ft_metric
  {
    const bote_objective k17[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {17, 0}}, k19[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {19, 0}},
                         far[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {BOTE_OBJ_MDTM, 10}},
                         absent[2] = {{BOTE_OBJ_MDTM, BOTE_SLOT_AF1}, {BOTE_OBJ_MDTM, BOTE_SLOT_FF2}};
    REFUSED(sweep(4, k17, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, unknown);
    REFUSED(sweep(4, k19, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, unknown);
    REFUSED(sweep(4, far, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, slot);
    REFUSED(sweep(3, absent, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, f2);
    // the kind before the slot of one objective
    const bote_objective both[1] = {{19, 99}}, mslot[1] = {{BOTE_OBJ_MDTM, 99}};
    REFUSED(sweep(4, both, 1, 4, nullptr, 0, 0), BOTE_E_ARG, unknown);
    REFUSED(sweep(4, mslot, 1, 4, nullptr, 0, 0), BOTE_E_ARG, slot);
    const bote_objective sm[2] = {{BOTE_OBJ_SCORE, 0}, {BOTE_OBJ_MDTM, BOTE_SLOT_AF1}};
    REFUSED(sweep(4, sm, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gmdtm);
    REFUSED(sweep(4, sm, 2, 4, &rp0, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, gmdtm);
    REFUSED(sweep(4, sm, 2, 4, nullptr, BOTE_KERNEL_FAST, 0), BOTE_E_ARG, need);
    REFUSED(sweep(4, sm, 2, 4, &rp0, BOTE_KERNEL_FAST, 0), BOTE_E_ARG, "bad ft_metric");
    ACCEPTED(sweep(4, sm, 2, 4, &rp, BOTE_KERNEL_FAST, 0));
  }
  // the key's bounds: the largest slot (4096 values) with half the values 0 and
  // half 2 * 16383 has the largest mean absolute deviation, half the range
  {
    const uint32_t c = BOTE_MAX_CLIENTS;
    std::vector<uint32_t> x(c, 0u);
    for (uint32_t i = c / 2; i < c; ++i) x[i] = 32766;
    const uint64_t H = mdtm_half_deviation(x.data(), c), S1 = (uint64_t)(c / 2) * 32766;
    CHECK(H == (uint64_t)c * c * 32766 / 4);
    CHECK(H < (1ull << 37) && S1 < (1ull << 27));
    uint64_t key = 0;
    CHECK(mdtm_key(H, S1, key) && key != ~0ull && (key >> 27) == H && (key & ((1ull << 27) - 1)) == S1);
    // every value at the maximum: the largest sum, H = 0
    std::vector<uint32_t> top(c, 32766u);
    CHECK(mdtm_half_deviation(top.data(), c) == 0);
    CHECK(mdtm_key(0, (uint64_t)c * 32766, key) && key == (uint64_t)c * 32766 && key < (1ull << 27) - 1);
    // a value at an integral mean is not above it; the direct sum on a small slot
    const uint32_t y[4] = {1, 2, 3, 2};  // S1 = 8, c = 4: only 3 is above (4 * 3 - 8 = 4)
    CHECK(mdtm_half_deviation(y, 4) == 4);
    const uint32_t z[3] = {0, 0, 1};  // S1 = 1, c = 3: 3 * 1 - 1 = 2; sum |c x - S1| = 1 + 1 + 2 = 2 H
    CHECK(mdtm_half_deviation(z, 3) == 2);
    // a half that does not fit is refused
    CHECK(!mdtm_key(1ull << 37, 0, key) && !mdtm_key(0, (1ull << 27) - 1, key));
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("mdtm host ok\n");
  return 0;
}
