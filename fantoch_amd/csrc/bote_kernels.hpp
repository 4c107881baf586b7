// bote_kernels.hpp — launch interface between the C ABI (bote_capi.hip) and
// the gfx950 kernels (one section per kernel file).
#pragma once
#include "bote_device.hpp"

namespace bote {

constexpr int NSLOT = 10;
constexpr int G_MERGE_LISTS = 8;  // lists merged per workgroup
enum { SLOT_AF1 = 0, SLOT_FF1 = 1, SLOT_AF2 = 2, SLOT_FF2 = 3, SLOT_E = 4 };
// (OBJ_MDTM lies between OBJ_MAX and OBJ_PCTL: tests on a kind are equalities,
// except `>= OBJ_PCTL`, the percentiles)
enum { OBJ_SCORE = 0, OBJ_MEAN = 1, OBJ_COV = 2, OBJ_MAX = 16, OBJ_MDTM = 18 };
// A percentile objective (BOTE_OBJ_PCTL) as the kernels see it in obj_kind:
// the host (bote_capi_sweep.hip, pctl_device_kind) turns bp and the slot's
// count into OBJ_PCTL | (whole ? PCTL_WHOLE : 0) | need, need = 1..PCTL_DEPTH:
// twice the percentile is 2 * (the need-th largest value of the slot), or with
// `whole` that value plus the (need - 1)-th largest.  Every other kind is
// below OBJ_PCTL.
constexpr uint32_t OBJ_PCTL = 0x10000u, PCTL_WHOLE = 16u, PCTL_NEED_MASK = 15u;
constexpr int PCTL_DEPTH = 8;       // the generic kernel's sorted list
constexpr int PCTL_FAST_DEPTH = 4;  // the fast kernel's list variant

struct EvalArgs {
  // planet (device): latency << 4, row = from
  const uint32_t* mat;
  uint32_t R;
  // server list (region ids; positions index it) and client list
  const uint32_t* srv;
  uint32_t ns;
  const uint32_t* cli;
  uint32_t nc;
  int srv_sorted;  // srv ascending => colex positions are already in name order
  // work: explicit configs (positions, n per config) or colex ranks
  const uint32_t* cfgs;
  // or an explicit device list of colex ranks whose length is read on the
  // device (the fast sweep's deferred near-tie configs): [0, *rank_count)
  const uint64_t* rank_list;
  const unsigned long long* rank_count;
  uint64_t rb, re;  // [rb, re) ranks, or config indices when cfgs != null
  uint32_t runlen;  // consecutive ranks per lane job
  const uint64_t* binom;  // (ns+1) x (n+1)
  // ranking params (compute_score)
  int want_score;
  double p_fmean, p_emean, p_fair;
  int ft_metric;
  // key set: 0 compute_stats' 10 slots; 1 the extended key set (slots
  // 10..19 and every leader's FPaxos moments; include/bote_hip.h)
  uint32_t keys;
  // FULL outputs (moments: NSLOT or, with keys, NSLOT_X per config)
  uint32_t* out_vals;
  uint32_t* out_leader;
  uint64_t* out_s1;
  uint64_t* out_s2;
  double* out_mean;
  double* out_cov;
  double* out_score;
  uint8_t* out_valid;
  uint64_t* out_al_s1;  // keys: ncfg x 2 x n, all leaders (f = 1, 2; config order)
  uint64_t* out_al_s2;
  // TOP-K outputs
  int n_obj;
  uint32_t obj_kind[MAXOBJ];
  uint32_t obj_slot[MAXOBJ];
  uint32_t K;
  Rec* out_top;                      // [grid][n_obj][KP]
  unsigned long long* out_counters;  // [0] valid count, [1] digest
  int want_digest;
  // overflow fallback of the fast sweep: when set, every block exits at once
  // unless *run_if_over > over_cap (the deferred-rank queue overflowed), so the
  // fallback is stream-ordered with no host round trip
  const unsigned long long* run_if_over;
  uint64_t over_cap;
};

struct SingleArgs {
  const uint32_t* mat;  // latency << 4
  uint32_t R;
  const uint32_t* servers;
  uint32_t ns;
  const uint32_t* clients;
  uint32_t nc;
  const uint32_t* froms;
  uint32_t nf;
  uint32_t q;
  uint32_t leader;
  int stat;
  uint64_t* out;
  uint32_t* out_pos;
  int* err;
};

// ---- fast-path sweep (bote_sweep.hip)
constexpr uint32_t FAST_BD = 256;
struct FastArgs {
  const uint2* cqt;  // client quads, column-major, column stride cq_stride uint2 (quad_stride)
  const uint2* rqt;  // region quads (rows = all regions), used when rq_separate
  int rq_separate;
  uint32_t R, cq_quads, rq_quads;
  uint32_t cq_stride, rq_stride;  // quads per column (>= quads + 1; an odd number of 16-B units)
  const uint32_t* srv;
  uint32_t ns;
  int srv_identity;  // srv[p] == p
  uint32_t nc;
  const uint64_t* binom;
  uint64_t rb, re;
  uint32_t runlen;
  uint32_t s2_flush;  // quads per 32-bit sum-of-squares chunk
  uint32_t g_flush;   // group kernel: quads per flush of its 32-bit square sums and packed-u16 sums
  uint32_t k_flush;   // group kernel, extended keys: quads per flush of its 32-bit sum of squared keys
  uint32_t gbd;       // group kernel: workgroup size (multiple of 64, <= 1024)
  uint32_t gqsh;      // group kernel: log2 of the qtab plane stride in bytes (1 << gqsh >= gbd * 4)
  uint32_t gslots;    // group kernel, n <= 7: client lines per wave (0: none), see bote_group.hip
  uint32_t grx;       // group kernel, n <= 7: per-group position table (1) or per-lane row sorts (0)
  uint32_t keys;      // group kernel: 1 = the extended key set (n = 4..7, default objectives first)
  uint32_t gbins;     // group kernel, base key set: the member-binned client loop (bote_group.hip BN)
  uint32_t s32;       // every sum of squares of a slot fits 32 bits (nc (2 max)^2 < 2^32): the SI group kernels keep them in 32 bits
  uint32_t v32;       // and every V = cnt s2 - s1^2 (cnt^2 (2 max)^2 < 2^32)
  // group kernel work distribution: nwchunks > 0: waves take cost-balanced
  // rank chunks [wchunks[c], wchunks[c+1]) from ticket counters (zeroed
  // before each launch); 0: each wave sweeps an equal share of ranks.  The
  // counter is sharded wshards ways (one 128-B line each, wctr[32 * x]):
  // blocks b with b % wshards == x take chunks x, x + wshards, ... (one
  // device-scope word saturates near 90 tickets per us, MI355X_MICROARCH.md)
  const uint64_t* wchunks;
  uint32_t nwchunks;
  unsigned int* wctr;
  uint32_t wshards;
  // per chunk, 4 u64: the colex rank of its first group's fixed positions,
  // then those positions as bytes (16 at most); null: unranked on the device
  const uint64_t* wstate;
  // top-K seed (bote_capi.hip launch_fast_path): the sample launch (smin
  // non-null) takes nwchunks chunks of ssteps steps at wchunks[c] and records, per
  // objective o, the least key of chunk c at smin[o * nwchunks + c] (no lists,
  // counters or deferrals); seed_kernel turns those into tseed[o], the K-th
  // least, a bound on the launch's K-th key that the main launch starts its
  // thresholds at
  // With smin_wave, the slot is the wave's (o * waves + wave, the least key
  // of the chunks it took): as many slots as waves, not chunks, for the seed
  // kernel to select from (K slots <= x are still K distinct configs <= x).
  uint64_t* smin;
  const uint64_t* tseed;
  uint32_t ssteps;  // sample launch: steps (of 64 configs) per sample chunk
  uint32_t smin_wave;
  // kbound (non-null: the one-launch merge follows): per objective the least
  // K-th key over the blocks' full lists (atomicMin at the list dump, reset by
  // zero_ctl); a block then writes only its records with keys <= that bound,
  // then a rec_max terminator, instead of n_obj x KP records
  unsigned long long* kbound;
  int want_score, p_int;
  int64_t p1i, p2i;  // p_int: min_mean_{fpaxos,epaxos}_improv * nc as integers
  // group kernel mean tests on D = the integer difference of two sums: true
  // above hi, false below lo, the reference's f64 arithmetic in [lo, hi]
  // (lo = hi = p1i when p_int; otherwise floor/ceil of p * nc -/+ 1)
  int32_t m1_lo, m1_hi, m2_lo, m2_hi;
  double p_fmean, p_emean;
  int ft_metric;
  int n_obj;
  uint32_t obj_kind[MAXOBJ];
  uint32_t obj_slot[MAXOBJ];
  uint32_t K;
  Rec* out_top;
  unsigned long long* out_counters;
  int want_digest;
  // group kernel (bote_group.hip): packed (p0 | p1 << 8 | p2 << 16) of the
  // 3-subsets of positions in colex order (the low part of a group's ranks)
  const uint32_t* lowtab;
  uint64_t* queue;  // deferred near-tie configs (colex ranks)
  unsigned long long* queue_count;
  uint64_t queue_cap;
#ifdef BOTE_DEBUG
  // Device-assert builds only (scripts/build_variant.sh debug -DBOTE_DEBUG):
  // failed bounds checks set bits in *dbg_flag (soft asserts: no trap, the
  // kernel keeps running) and bote_sweep_result reports BOTE_E_DEVICE.
  unsigned int* dbg_flag;
  uint64_t lowtab_n;  // entries of lowtab
#endif
#ifdef BOTE_PATHSTATS
  // Path-statistics builds only (scripts/build_variant.sh pstats -DBOTE_PATHSTATS,
  // scripts/pathstats.py): per wave-step, how often each rare path of the group
  // kernel runs for the wavefront (any lane taking it), 64 counters
  unsigned long long* pstats;
#endif
#ifdef BOTE_ABLATION
  // Timing-diagnostics builds only (scripts/build_variant.sh NAME -DBOTE_ABLATION,
  // env BOTE_ABLATE; results are wrong when set).  The product library is
  // compiled without it: ABLATE() is the constant false there.
  // 1 skip client loop, 2 skip Q phase, 4 skip top-K step, 8 skip score, 16 skip digest;
  // group kernel: 32 skip variable-row sorts, 64 skip fixed-row insertions,
  // 128 skip leader selection, 256 skip validity, 512 skip colocated FPaxos
  uint32_t ablate;
#endif
};
// A pinned sweep's fixed members (bote_pinned.hpp).  The launchers of the fast
// and the generic kernel take a pointer to it (null: not pinned), run their
// pinned variant and append it to the kernel's arguments.
// lim: a bounded batch's limits (DESIGN.md §4 "Streaming evolving search"),
// exclusive, on the config's S1 of SLOT_AF1 and SLOT_AF2: one more term of
// compute_score validity, S1 < lim.  PIN_NO_BOUND passes every sum (S1 < 2^27).
// The batch variant of the fast kernel and the pinned variant of the generic
// kernel read them; PIN_NONE and PIN_ONE never do.  The last words of every
// kernarg struct that ends in a PinArgs.
constexpr uint32_t PIN_NO_BOUND = 0xFFFFFFFFu;
struct PinArgs {
  uint32_t pin_n;      // m
  uint32_t pin[MAXN];  // the pinned positions, ascending; 0 from pin_n on
  uint32_t lim[2] = {PIN_NO_BOUND, PIN_NO_BOUND};
};
// A batch of pinned sweeps (DESIGN.md §4 "Batched pinned sweeps"): n_sets
// pinned sets of one size, each swept over its whole pinned-rank space in one
// launch of the fast kernel's batch variant.  The work is cut into units
// (set b, slice s), unit u = b * slices + s, slice s being the pinned ranks
// [s * slice_len, min((s + 1) * slice_len, ptotal)); a workgroup walks units
// blockIdx.x, += gridDim.x.  Unit u's lists go to list slot b * BATCH_SET_LISTS
// + s of out_top, set b's valid count and digest to out_counters[2 b .. 2 b + 1].
// Deferred configs are only counted (queue_count): a batch that deferred any is
// recomputed set by set on the generic kernel when its result is fetched.
constexpr uint32_t BATCH_SET_LISTS = G_MERGE_LISTS;         // list slots per set: one merge group
constexpr uint32_t BATCH_MAX_SLICES = BATCH_SET_LISTS - 1;  // (one slot is kept for a per-set fix-up list)
struct BatchArgs {
  const PinArgs* sets;  // [n_sets], positions ascending
  uint32_t n_sets, slices;
  uint64_t slice_len, ptotal;
  uint32_t runlen;  // consecutive pinned ranks per lane job of a unit
};
// the fast kernel's member stage (bote_sweep.hip Members).  Plain ints, not
// enumerators of an unnamed enum: where one appears in a kernel's signature the
// host and the device pass number the enum differently, the mangled names
// differ and the runtime does not find the kernel.
constexpr int PIN_NONE = 0, PIN_ONE = 1, PIN_BATCH = 2;
// A census launch (DESIGN.md §4 "Census sweeps", bote_census.hpp): per
// objective T thresholds, ascending in (key, rank), and the counts they add to.
// The census variants of the fast and the generic kernel take it at the end of
// their arguments.
constexpr int CENSUS_T = 16;  // thresholds per objective of a launch, at most
struct CensusArgs {
  const Rec* thr;             // [n_obj][T]
  uint32_t T;                 // 1 .. CENSUS_T
  unsigned long long* below;  // [n_obj][T]: += the configs before each threshold
};
// A constrained sweep (DESIGN.md §4 "Constrained sweeps"): the launch's key
// entries [0, n_lists) are its objectives, the entries [n_lists, n_obj) of
// obj_kind / obj_slot its constraints, whose keys the kernels build like any
// objective's.  A config is admitted when key[o] <= bound[o] for every
// constraint entry o; only an admitted config offers its keys to the lists, and
// the admitted configs are counted into *admitted.  The constrained variants of
// the fast and the generic kernel take it at the end of their arguments; they
// size their LDS for n_obj lists and write, merge and dump n_lists.
struct ConArgs {
  uint32_t n_lists;
  uint64_t bound[MAXOBJ];         // by key entry; read from n_lists on
  unsigned long long* admitted;   // += the admitted configs of the launch
};
// the kernels' arguments with it at the end (the kernarg offsets of FastArgs and EvalArgs stay)
struct ConFastArgs : FastArgs {
  ConArgs cz;
};
struct ConEvalArgs : EvalArgs {
  ConArgs cz;
};
// Where the constrained variants keep the bounds: both kernels' block top-K has
// MAXOBJ threshold records (TopkLds::thr) and touches only those of its lists,
// so the rank word of record o >= n_lists holds bound[o] (its key word stays
// all ones, "no threshold", for the key builders that screen against it).  The
// bounds are read back per config from LDS, not kept in registers.
#ifdef __HIPCC__
// the entries that have a list: all of them, or a constrained variant's first n_lists (read where
// it is used, as a.n_obj is: the other instantiations keep their code)
template <bool CON, class Args>
__device__ __forceinline__ int list_count(const Args& a) {
  if constexpr (CON) return (int)a.cz.n_lists;
  else return a.n_obj;
}
// every thread of the block, after topk_init and its barrier; the caller's next barrier publishes the bounds
__device__ __forceinline__ void con_init(const TopkLds& t, const ConArgs& z) {
  if (threadIdx.x < (uint32_t)MAXOBJ && threadIdx.x >= z.n_lists) t.thr[threadIdx.x].rank = z.bound[threadIdx.x];
}
// An evaluated config's verdict, from its n_keys keys: admitted when every
// constraint key was built and lies within its bound (inclusive); a rejected
// config withdraws every offer.
__device__ __forceinline__ bool con_admit(const TopkLds& t, int n_lists, int n_keys, const uint64_t (&key)[MAXOBJ],
                                          bool (&ok)[MAXOBJ]) {
  bool adm = true;
#pragma unroll
  for (int o = 0; o < MAXOBJ; ++o)
    if (o >= n_lists && o < n_keys) adm = adm && ok[o] && key[o] <= t.thr[o].rank;
#pragma unroll
  for (int o = 0; o < MAXOBJ; ++o) ok[o] = ok[o] && adm;
  return adm;
}
#endif
#ifdef BOTE_DEBUG
// bit `code` of *dbg_flag when `cond` fails (codes: DESIGN.md §5, debug build)
#define GASSERT(a, cond, code)                                                    \
  do {                                                                            \
    if (!(cond)) atomicOr((a).dbg_flag, 1u << (code));                            \
  } while (0)
#else
#define GASSERT(a, cond, code) \
  do {                         \
  } while (0)
#endif
#ifdef BOTE_PATHSTATS
// counter k += 1 when any active lane of the wavefront has `cond` (one lane adds)
#define PSTAT(a, k, cond)                                                                        \
  do {                                                                                           \
    const unsigned long long pm_ = __ballot(cond), pa_ = __ballot(1);                            \
    if (pm_ && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(pa_)) atomicAdd(&(a).pstats[k], 1ull); \
  } while (0)
#else
#define PSTAT(a, k, cond) \
  do {                    \
  } while (0)
#endif
#ifdef BOTE_ABLATION
#define ABLATE(a, bit) (((a).ablate & (bit)) != 0)
#else
#define ABLATE(a, bit) false
#endif
// `tail`: the variant of the fast kernel.  FAST_PLAIN treats no MAX or
// percentile objective; FAST_MAX also carries every slot's maximum (the worst
// client) for BOTE_OBJ_MAX objectives; FAST_LIST carries every slot's
// PCTL_FAST_DEPTH largest values, descending, for percentile objectives of
// need <= PCTL_FAST_DEPTH (entry 0 serves the MAX objectives of such a sweep);
// FAST_MDTM treats BOTE_OBJ_MDTM objectives (a second pass over the clients
// against each slot's mean) and carries no maxima or lists: a sweep with an
// MDTM objective beside a MAX or percentile one runs the generic kernel
enum { FAST_PLAIN = 0, FAST_MAX = 1, FAST_LIST = 2, FAST_MDTM = 3 };
// (census: the census variant, FAST_PLAIN and unpinned: thresholds and bins in place of the lists)
size_t fast_smem_bytes(const FastArgs& a, uint32_t n, int tail, bool census = false);
// (pin: PIN_*; the pinned and the batch variant are FAST_PLAIN only: SCORE, MEAN and COV objectives)
// (con: the constrained variant, unpinned; fast_has_constrained: whether it is built for `tail`)
int fast_occupancy(uint32_t n, int tail, int pin, size_t shm, bool census = false, bool con = false);
bool fast_has_constrained(uint32_t n, int tail);
// (e0, e1: events carried by the dispatch itself, bote_launch.hpp, for a timed launch)
hipError_t launch_fast(const FastArgs& a, uint32_t n, int tail, const PinArgs* pin, uint32_t grid, size_t shm,
                       hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the batch variant (FAST_PLAIN) over the units of `b`; a.rb, a.re and a.runlen are not read
hipError_t launch_fast_batch(const FastArgs& a, uint32_t n, const BatchArgs& b, uint32_t grid, size_t shm,
                             hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the census variant (FAST_PLAIN, unpinned) over [a.rb, a.re): adds to z.below, a.out_counters[0]
// and the deferred queue; a.out_top and a.K are not read
hipError_t launch_fast_census(const FastArgs& a, uint32_t n, const CensusArgs& z, uint32_t grid, size_t shm,
                              hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the constrained variant (unpinned) over [a.rb, a.re): a.n_obj counts the objectives and the
// constraints, z.n_lists lists per block go to a.out_top
hipError_t launch_fast_con(const FastArgs& a, uint32_t n, int tail, const ConArgs& z, uint32_t grid, size_t shm,
                           hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
size_t group_smem_bytes(const FastArgs& a, uint32_t n);
bool group_uses_lines(uint32_t n);  // n <= 7: client lines (FastArgs::gslots) and register lookups
// the extended key set's group kernels target BOTE_GROUP_WAVES_XK waves per
// SIMD and are bounded to workgroups of that many waves per SIMD
// (GROUP_XK_MAX_BD); the capi's eligibility probe and its geometry loop share
// it. 4 (128 VGPRs, 404 B/lane scratch) beats 3 (168 VGPRs, 252 B/lane) on
// config 5: 186.1 / 185.8 ms vs 198.3 / 197.9 ms kernel, same valid count and
// digest (profiles/r05r: DESIGN.md §5)
#ifndef BOTE_GROUP_WAVES_XK
#define BOTE_GROUP_WAVES_XK 4
#endif
constexpr uint32_t GROUP_XK_MAX_BD = 256 * BOTE_GROUP_WAVES_XK;
bool group_supports_keys(uint32_t n, uint32_t bd);  // the extended key set on the group kernel (n = 4..7, bd <= GROUP_XK_MAX_BD)
// workgroups per CU of the kernel instantiation launch_group runs for `a`
// (workgroup size a.gbd)
int group_occupancy(const FastArgs& a, uint32_t n, size_t shm, bool def_objectives);
hipError_t launch_group(const FastArgs& a, uint32_t n, bool def_objectives, uint32_t grid, size_t shm, hipStream_t st,
                        hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// ---- generic exact kernel (bote_eval.hpp; its family units bote_eval_*.hip; launchers in bote_kernels.hip)
size_t eval_smem_bytes(const EvalArgs& a, uint32_t n, uint32_t bd, bool topk);
// The generic kernel's top-K instantiations by the passes a sweep's objectives
// add to a config (each level has the ones below it): EVAL_PCTL one pass per
// percentile objective, EVAL_MDTM also one per MDTM objective.  Sweeps with
// neither, and full outputs, take EVAL_PLAIN and keep their code and registers.
enum { EVAL_PLAIN = 0, EVAL_PCTL = 1, EVAL_MDTM = 2 };
inline int eval_passes(const uint32_t* obj_kind, int n_obj) {
  int e = EVAL_PLAIN;
  for (int o = 0; o < n_obj; ++o)
    e = obj_kind[o] == OBJ_MDTM ? (int)EVAL_MDTM : obj_kind[o] >= OBJ_PCTL && e < EVAL_PCTL ? (int)EVAL_PCTL : e;
  return e;
}
// (passes: the top-K instantiation launch_eval takes for the sweep's objectives, eval_passes)
// (pin: the pinned variant, a top-K sweep of the base key set in the
// rank-range mode, [a.rb, a.re) being pinned ranks: the generic path, the fast
// sweep's overflow fallback, and MAX / percentile / MDTM objectives.  It has
// EVAL_PLAIN and EVAL_MDTM; a percentile sweep takes EVAL_MDTM)
int eval_occupancy(uint32_t n, bool full, uint32_t bd, size_t shm, bool keys = false, int passes = EVAL_PLAIN,
                   bool pin = false, bool census = false, bool con = false);
hipError_t launch_eval(const EvalArgs& a, uint32_t n, bool full, uint32_t grid, uint32_t bd, size_t shm,
                       hipStream_t st, const PinArgs* pin = nullptr);
// The census variant (base keys; EVAL_PLAIN, or EVAL_MDTM for a MAX, percentile
// or MDTM objective) over the ranks [a.rb, a.re) or the rank list a.rank_list:
// adds to z.below and a.out_counters[0]; a.out_top and a.K are not read, shm is
// eval_smem_bytes with top-K structures.  On a rank list longer than a.re -
// a.rb (the queue overflowed: the fallback counts the range) it counts nothing.
hipError_t launch_eval_census(const EvalArgs& a, uint32_t n, const CensusArgs& z, uint32_t grid, uint32_t bd,
                              size_t shm, hipStream_t st, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// The constrained variant (base keys, unpinned, top-K; EVAL_PLAIN, or EVAL_MDTM
// for a percentile or MDTM entry) over the ranks [a.rb, a.re) or the rank list:
// a.n_obj counts the objectives and the constraints, shm is sized for that many
// lists, and z.n_lists lists per block go to a.out_top
hipError_t launch_eval_con(const EvalArgs& a, uint32_t n, const ConArgs& z, uint32_t grid, uint32_t bd, size_t shm,
                           hipStream_t st);
// A census launch's start: the n = n_obj x T thresholds (host memory, read before
// the call returns) into the device table thr, and below[0 .. n), counters[0 .. 1]
// and, where given, below_alt, counters_alt and *qcount zeroed
hipError_t launch_census_begin(const Rec* host_thr, uint32_t n, Rec* thr, unsigned long long* below,
                               unsigned long long* below_alt, unsigned long long* counters,
                               unsigned long long* counters_alt, unsigned long long* qcount, hipStream_t st);
// dst[0 .. n) = (sel && *sel > cap ? alt : src)[0 .. n), then dst[n] = the same choice
// of csrc[0] / calt[0] (a census's counts and its valid count; alt, calt null without sel)
hipError_t launch_census_pick(const unsigned long long* src, const unsigned long long* alt, uint32_t n,
                              const unsigned long long* csrc, const unsigned long long* calt,
                              const unsigned long long* sel, uint64_t cap, uint64_t* dst, hipStream_t st);

// ---- top-K lists: merge, seed, counters (bote_merge.hip)
// One level of the merge tree: every G_MERGE_LISTS lists of `src` (n_lists
// lists, list i of objective o at src[i * list_stride + o * KP]) into one at
// dst[g * out_stride + o * KP].  With `sel` the input is chosen on the
// device: `alt` (alt_lists lists) when *sel > cap, else `src`; a plain merge
// passes null, 0 for alt, alt_lists, sel and cap.
hipError_t launch_merge(const Rec* src, uint32_t n_lists, const Rec* alt, uint32_t alt_lists, uint64_t list_stride,
                        const unsigned long long* sel, uint64_t cap, Rec* dst, uint64_t out_stride, uint32_t n_obj,
                        hipStream_t st);
constexpr uint32_t WIDE_MERGE_LISTS = 4096;
// one launch for a sweep's block lists (<= WIDE_MERGE_LISTS lists): the K least per
// objective into dst[o * KP] (sel/alt/cap: the overflow fallback's choice)
// csrc/calt/cdst: the counters (valid, digest) copied to cdst by the same
// device choice (sel) as the lists, as launch_pick_counters does
hipError_t launch_merge_wide(const Rec* src, uint32_t n_lists, const Rec* alt, uint32_t alt_lists, uint64_t list_stride,
                             const unsigned long long* sel, uint64_t cap, const unsigned long long* kbound, Rec* dst,
                             uint32_t n_obj, uint32_t K, const unsigned long long* csrc, const unsigned long long* calt,
                             uint64_t* cdst, hipStream_t st);
// a fast-path sweep's per-launch control words zeroed (kbound: set to no bound)
hipError_t launch_zero_ctl(unsigned long long* counters, unsigned long long* qcount, unsigned int* wctr,
                           unsigned long long* counters_alt, unsigned long long* kbound, hipStream_t st);
// tseed[o] = the K-th least of smin[o * nsamp .. + nsamp) (FastArgs::smin), all-ones when nsamp < K
hipError_t launch_seed(const uint64_t* smin, uint32_t nsamp, uint32_t n_obj, uint32_t K, uint64_t* tseed,
                       hipStream_t st);
// dst[0..1] = (*sel > cap ? alt : src)[0..1]
hipError_t launch_pick_counters(const unsigned long long* src, const unsigned long long* alt,
                                const unsigned long long* sel, uint64_t cap, uint64_t* dst, hipStream_t st);
// dst[0..1] = the sum over i < n of src[i * stride + off + 0..1]
hipError_t launch_sum_counters(const uint64_t* src, uint32_t n, uint64_t stride, uint64_t off, uint64_t* dst,
                               hipStream_t st);

// ---- leaderless latencies for several quorum sizes (bote_quorums.hip)
struct LqArgs {
  const uint32_t* mat;  // latency << 4
  uint32_t R;
  const uint32_t* srv;
  uint32_t ns;
  const uint32_t* cli;
  uint32_t nc;
  const uint32_t* cfgs;  // ncfg x n positions, or null (colex ranks from rank_begin)
  const uint64_t* binom;
  uint64_t rank_begin, ncfg;
  const uint32_t* qs;  // nq quorum sizes, each in [1, n]
  uint32_t nq;
  uint32_t* out_vals;   // ncfg x nq x (nc + n)
  uint64_t* out_sum;    // ncfg x nq x 2 (Input, Colocated)
  uint64_t* out_sumsq;  // ncfg x nq x 2
};
size_t lq_smem_bytes(const LqArgs& a, uint32_t n);
hipError_t launch_leaderless_q(const LqArgs& a, uint32_t n, uint32_t grid, size_t shm, hipStream_t st);

// ---- Search::sorted_evolving_configs on the device (bote_chain.hip)
struct ChainHostLevel {
  uint32_t cnt, n;
  const uint64_t* mask;
  const double* score;
  const double* mean;
};
hipError_t chain_search(const ChainHostLevel* lv, uint32_t ns, int ft_metric, double min_dec, uint64_t max_out,
                        uint32_t* out_idx, double* out_score, uint64_t* out_total, hipStream_t st, int* too_many);

// ---- the per-call Bote::* API (bote_kernels.hip)
hipError_t launch_single(const SingleArgs& a, int mode, hipStream_t st);
hipError_t launch_best_leader(const SingleArgs& a, const uint64_t* vals, double* stat, hipStream_t st);

}  // namespace bote
