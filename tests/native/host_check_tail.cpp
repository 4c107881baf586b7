// host_check_tail.cpp — the MAX (worst-client) objective in the argument
// checks of bote_sweep_create_keys (fantoch_amd/csrc/bote_host.cpp,
// check_sweep_args), under ASan + UBSan on the CPU: built and run by
// tests/test_tail_host.py.  R = 8 = ns = nc throughout.
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

int main() {
  const uint32_t id[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  const bote_ranking_params rp{110.0, 35.0, 0.0, 15.0, BOTE_FT_F1F2}, rp0{110.0, 35.0, 0.0, 15.0, 0};
  bool sc = false;
  auto sweep = [&](uint32_t n, const bote_objective* o, uint32_t n_obj, uint32_t K, const bote_ranking_params* r,
                   int kernel, uint32_t keys) { return check_sweep_args(8, id, 8, id, 8, n, o, n_obj, K, r, kernel, keys, sc); };
  const char *unknown = "unknown objective kind", *slot = "slot out of range",
             *f2 = "slot does not exist for this n (max_f < 2)", *need = "SCORE objective needs ranking params",
             *group = "the group kernel does not compute MAX objectives (fast or generic kernel)";
  static_assert(BOTE_OBJ_MAX == 16, "the MAX objective kind");

  // kind 16 with every existing slot of either key set, on auto, generic and fast
  for (uint32_t keys = 0; keys <= 1; ++keys)
    for (uint32_t n = 2; n <= 8; ++n)
      for (uint32_t s = 0; s < (keys ? BOTE_NSLOTS_X : BOTE_NSLOTS); ++s) {
        const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, s}};
        for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) {
          if (slot_exists_n(n, s, keys)) ACCEPTED(sweep(n, o, 2, 100, nullptr, kernel, keys));
          else REFUSED(sweep(n, o, 2, 100, nullptr, kernel, keys), BOTE_E_ARG, f2);  // MAX on a slot absent for n
        }
      }
  {
    const bote_objective o[1] = {{BOTE_OBJ_MAX, BOTE_SLOT_FF1}};
    ACCEPTED(sweep(4, o, 1, 1, nullptr, BOTE_KERNEL_AUTO, 0));
    if (sc) {
      std::printf("a MAX objective reported as SCORE\n");
      ++failures;
    }
  }
  // the neighbouring kinds stay unknown
  for (uint32_t kind : {3u, 4u, 15u, 17u, 32u, 0xFFFFFFFFu}) {
    const bote_objective o[2] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}, {kind, BOTE_SLOT_AF1}};
    for (uint32_t keys = 0; keys <= 1; ++keys) REFUSED(sweep(4, o, 2, 4, nullptr, BOTE_KERNEL_AUTO, keys), BOTE_E_ARG, unknown);
  }
  // the slot range and slot existence apply to MAX as to MEAN
  {
    const bote_objective s10[1] = {{BOTE_OBJ_MAX, 10}}, s20[1] = {{BOTE_OBJ_MAX, 20}},
                         a2[1] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF2}}, fl2[1] = {{BOTE_OBJ_MAX, BOTE_SLOT_FL2}};
    REFUSED(sweep(4, s10, 1, 4, nullptr, 0, 0), BOTE_E_ARG, slot);
    ACCEPTED(sweep(4, s10, 1, 4, nullptr, 0, 1));
    REFUSED(sweep(4, s20, 1, 4, nullptr, 0, 1), BOTE_E_ARG, slot);
    REFUSED(sweep(3, a2, 1, 4, nullptr, 0, 0), BOTE_E_ARG, f2);
    ACCEPTED(sweep(4, a2, 1, 4, nullptr, 0, 0));
    REFUSED(sweep(3, fl2, 1, 4, nullptr, 0, 1), BOTE_E_ARG, f2);
  }
  // a forced group kernel refuses MAX, with either key set; without MAX it is accepted
  {
    const bote_objective o[2] = {{BOTE_OBJ_MEAN, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}};
    REFUSED(sweep(4, o, 2, 100, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, group);
    REFUSED(sweep(4, o, 2, 100, &rp, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, group);
    ACCEPTED(sweep(4, o, 1, 100, nullptr, BOTE_KERNEL_GROUP, 0));
  }
  // order: key set, kernel path, lists, count, null, K, then per objective
  // kind, slot range, slot existence; then group + MAX, SCORE's params, ft_metric
  {
    const bote_objective mx[1] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}};
    REFUSED(sweep(4, mx, 1, 4, nullptr, BOTE_KERNEL_GROUP, 2), BOTE_E_ARG, "unknown key set");
    REFUSED(sweep(4, mx, 1, 4, nullptr, 4, 0), BOTE_E_ARG, "unknown kernel path");
    REFUSED(sweep(9, mx, 1, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, "config size larger than the server list");
    REFUSED(sweep(4, mx, 9, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_RANGE, "more than 8 objectives");
    REFUSED(sweep(4, nullptr, 1, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, "objectives null");
    REFUSED(sweep(4, mx, 1, 0, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_RANGE, "K must be in [1, 128]");
    // a later objective's bad kind, slot or absent slot comes before the group refusal
    const bote_objective k17[2] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}, {17, 0}}, far[2] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, 10}},
                         absent[2] = {{BOTE_OBJ_MAX, BOTE_SLOT_AF1}, {BOTE_OBJ_MAX, BOTE_SLOT_FF2}};
    REFUSED(sweep(4, k17, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, unknown);
    REFUSED(sweep(4, far, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, slot);
    REFUSED(sweep(3, absent, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, f2);
    // the kind before the slot of one objective
    const bote_objective both[1] = {{15, 99}};
    REFUSED(sweep(4, both, 1, 4, nullptr, 0, 0), BOTE_E_ARG, unknown);
    // group + MAX before SCORE's params and the ft_metric
    const bote_objective sm[2] = {{BOTE_OBJ_SCORE, 0}, {BOTE_OBJ_MAX, BOTE_SLOT_AF1}};
    REFUSED(sweep(4, sm, 2, 4, nullptr, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, group);
    REFUSED(sweep(4, sm, 2, 4, &rp0, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, group);
    REFUSED(sweep(4, sm, 2, 4, nullptr, BOTE_KERNEL_FAST, 0), BOTE_E_ARG, need);
    REFUSED(sweep(4, sm, 2, 4, &rp0, BOTE_KERNEL_FAST, 0), BOTE_E_ARG, "bad ft_metric");
    ACCEPTED(sweep(4, sm, 2, 4, &rp, BOTE_KERNEL_FAST, 0));
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("tail host ok\n");
  return 0;
}
