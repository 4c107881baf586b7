// host_check_constrained.cpp — constrained sweeps (bote_sweep_create_constrained)
// in the host code (fantoch_amd/csrc/bote_host.cpp): every refusal of
// check_constraint_args in its order, and the fast kernel's variant over the
// union of the objectives' and the constraints' kinds (fast_tail_plan), under
// ASan + UBSan on the CPU: built and run by tests/test_constrained_host.py.
// nc = 20 clients throughout.
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

// a percentile kind as the kernels take it, for slot `slot` of an n-config with 20 clients
static uint32_t dev_pctl(uint32_t bp, uint32_t slot, uint32_t n) {
  return DEV_KIND_PCTL | percentile_need(bp, slot_count(slot, 20, n));
}

int main() {
  const char *null_list = "constraints null", *unknown = "unknown constraint kind",
             *score = "SCORE is not a constraint kind", *range = "constraint slot out of range",
             *f2 = "constraint slot does not exist for this n (max_f < 2)",
             *need = "percentile constraint needs more than 8 of the slot's largest values",
             *many = "more than 8 objectives and constraints", *xk = "constrained sweeps compute the base key set",
             *group = "the group kernel does not apply constraints (fast or generic kernel)";
  const uint64_t all = ~0ull;
  auto check = [&](uint32_t n, const bote_constraint* c, uint32_t n_con, uint32_t n_obj, int kernel, uint32_t keys) {
    return check_constraint_args(20, n, c, n_con, n_obj, kernel, keys);
  };
  static_assert(sizeof(bote_constraint) == 16, "two words and the key");

  // ---- accepted: none at all (whatever the kernel and the key set), and every kind on every slot that exists
  ACCEPTED(check(5, nullptr, 0, 8, BOTE_KERNEL_GROUP, 1));
  for (uint32_t n = 2; n <= 8; ++n)
    for (uint32_t s = 0; s < BOTE_NSLOTS; ++s)
      for (uint32_t kind : {(uint32_t)BOTE_OBJ_MEAN, (uint32_t)BOTE_OBJ_COV, (uint32_t)BOTE_OBJ_MAX,
                            (uint32_t)BOTE_OBJ_MDTM, (uint32_t)BOTE_OBJ_PCTL(9900)}) {
        const bote_constraint c[1] = {{kind, s, 12345}};
        for (int kernel : {BOTE_KERNEL_AUTO, BOTE_KERNEL_GENERIC, BOTE_KERNEL_FAST}) {
          if (slot_exists_n(n, s, 0)) ACCEPTED(check(n, c, 1, 5, kernel, 0));
          else REFUSED(check(n, c, 1, 5, kernel, 0), BOTE_E_ARG, f2);
        }
      }

  // ---- the refusals, each with every later one also present: the first in order is reported
  {
    const bote_constraint bad[9] = {{17, 99, all}, {0, 99, all}, {1, 99, all}, {1, 2, all}, {BOTE_OBJ_PCTL(5000), 0, all},
                                    {1, 0, all},   {1, 0, all},  {1, 0, all},  {1, 0, all}};
    REFUSED(check(3, nullptr, 9, 8, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, null_list);
    REFUSED(check(3, bad, 9, 8, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, unknown);      // kind 17 is not defined
    REFUSED(check(3, bad + 1, 8, 8, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, score);    // SCORE, whatever its slot
    REFUSED(check(3, bad + 2, 7, 8, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, range);    // slot 99
    REFUSED(check(3, bad + 3, 6, 8, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, f2);       // af2 at n = 3
    REFUSED(check(3, bad + 4, 5, 8, BOTE_KERNEL_GROUP, 0), BOTE_E_RANGE, need);   // the median of 20 clients needs 11
    REFUSED(check(3, bad + 5, 4, 8, BOTE_KERNEL_GROUP, 1), BOTE_E_RANGE, many);   // 8 + 4
    REFUSED(check(3, bad + 5, 1, 7, BOTE_KERNEL_GROUP, 1), BOTE_E_ARG, xk);       // 7 + 1 fits; the extended key set
    REFUSED(check(3, bad + 5, 1, 7, BOTE_KERNEL_GROUP, 0), BOTE_E_ARG, group);
    ACCEPTED(check(3, bad + 5, 1, 7, BOTE_KERNEL_FAST, 0));
  }
  {  // kinds 3..15, 17, 19.. and a percentile of 0 or 10000 basis points are unknown
    for (uint32_t kind : {3u, 15u, 17u, 19u, 0x10000u, 0x10000u | 10000u, 0x20001u}) {
      const bote_constraint c[1] = {{kind, 0, 0}};
      REFUSED(check(5, c, 1, 1, BOTE_KERNEL_AUTO, 0), BOTE_E_ARG, unknown);
    }
    // the count: 7 + 2 is refused, 6 + 2 and 0 + 8 fit
    const bote_constraint c[8] = {{1, 0, 1}, {1, 1, 1}, {1, 4, 1}, {2, 0, 1}, {2, 1, 1}, {2, 4, 1}, {16, 0, 1}, {18, 0, 1}};
    REFUSED(check(5, c, 2, 7, BOTE_KERNEL_AUTO, 0), BOTE_E_RANGE, many);
    ACCEPTED(check(5, c, 2, 6, BOTE_KERNEL_AUTO, 0));
    ACCEPTED(check(5, c, 8, 0, BOTE_KERNEL_GENERIC, 0));
    REFUSED(check(5, c, 8, 1, BOTE_KERNEL_GENERIC, 0), BOTE_E_RANGE, many);
    // a percentile of a colocated slot (n values) needing at most 8 is fine where the clients' is not
    const bote_constraint p50c[1] = {{BOTE_OBJ_PCTL(5000), 5, 1}}, p50[1] = {{BOTE_OBJ_PCTL(5000), 0, 1}};
    ACCEPTED(check(5, p50c, 1, 1, BOTE_KERNEL_AUTO, 0));
    REFUSED(check(5, p50, 1, 1, BOTE_KERNEL_AUTO, 0), BOTE_E_RANGE, need);
  }

  // ---- routing over the union of kinds: the entries are the objectives, then the constraints
  {
    const uint32_t M = BOTE_OBJ_MEAN, CV = BOTE_OBJ_COV, S = BOTE_OBJ_SCORE, MX = BOTE_OBJ_MAX, MD = BOTE_OBJ_MDTM;
    const uint32_t p95 = dev_pctl(9500, 0, 5), p99 = dev_pctl(9900, 0, 5), p70 = dev_pctl(7000, 0, 5);
    CHECK((p95 & DEV_PCTL_NEED_MASK) == 2 && (p99 & DEV_PCTL_NEED_MASK) == 1 && (p70 & DEV_PCTL_NEED_MASK) == 7);
    auto plan = [](std::vector<uint32_t> kinds) { return fast_tail_plan(kinds.data(), (uint32_t)kinds.size()); };
    TailPlan t = plan({});
    CHECK(t.tail == TAIL_PLAIN && t.need == 0 && !t.mixed);
    t = plan({S, M, CV, /* constraints */ M, CV});
    CHECK(t.tail == TAIL_PLAIN && !t.mixed);
    t = plan({S, M, /* constraints */ MX});  // a MAX in the union: the fast kernel carries maxima
    CHECK(t.tail == TAIL_MAX && t.need == 0 && !t.mixed);
    t = plan({M, MX, /* constraints */ p95, MX});  // a percentile in the union: lists, which serve MAX too
    CHECK(t.tail == TAIL_LIST && t.need == 2 && !t.mixed);
    t = plan({M, /* constraints */ p99, p95});
    CHECK(t.tail == TAIL_LIST && t.need == 2 && !t.mixed);
    t = plan({M, /* constraints */ p70});  // a need of 5..8: the caller sends it to the generic kernel
    CHECK(t.tail == TAIL_LIST && t.need == 7 && t.need > 4 && !t.mixed);
    t = plan({M, /* constraints */ MD});  // an MDTM in the union: the MDTM variant
    CHECK(t.tail == TAIL_MDTM && !t.mixed);
    t = plan({MX, /* constraints */ MD});  // MDTM beside MAX: the generic kernel
    CHECK(t.tail == TAIL_MDTM && t.mixed);
    t = plan({MD, /* constraints */ MX});
    CHECK(t.tail == TAIL_MDTM && t.mixed);
    t = plan({M, /* constraints */ MD, p95});  // MDTM beside a percentile
    CHECK(t.tail == TAIL_MDTM && t.mixed && t.need == 2);
    // the decision does not depend on which side of the split a kind stands
    for (uint32_t a : {M, MX, MD, p95})
      for (uint32_t b : {M, MX, MD, p95}) {
        const TailPlan x = plan({a, b}), y = plan({b, a});
        CHECK(x.tail == y.tail && x.need == y.need && x.mixed == y.mixed);
      }
  }

  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("constrained host ok\n");
  return 0;
}
