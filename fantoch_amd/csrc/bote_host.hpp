// bote_host.hpp — host-only pieces of libbote_hip.so (plain C++, no HIP): the
// combinatorics of colex ranks, the group walk behind the cost-balanced work
// chunks and shard splits, the client-quad layouts, the fast-path eligibility
// test, the sweep planning (the exactness limits and flush counts of the fast
// kernels, the score bands, the compiled-in objective set, the chunk states
// and the top-K seed's sample plan), the result-block unpacking and the
// argument checks of the C ABI.  Compiled by g++ into the library and,
// separately, under ASan/UBSan by tests/test_sanitize.py (tests/native/
// host_check.cpp), so the driver's host code runs under the sanitizers the
// oracle does.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bote_hip.h"  // (codes, limits, bote_objective, bote_ranking_params: plain C)

namespace bote {
namespace host {

// C(m, k) as u64 (0 when k > m or on overflow).
uint64_t binom_u64(uint32_t m, uint32_t k);
// (ns + 1) x (n + 1) table, row m, column k: C(m, k).
std::vector<uint64_t> binom_table(uint32_t ns, uint32_t n);
// rank -> n ascending positions < ns (colex: rank = sum_j C(p_j, j + 1)).
// False when rank >= C(ns, n).
bool colex_unrank(uint64_t rank, uint32_t n, uint32_t ns, uint32_t* out);
uint64_t colex_rank(const uint32_t* pos, uint32_t n);

// ---------------------------------------------------------- pinned sweeps --
// A pinned sweep ranks the supersets of m pinned positions: its rank space is
// the colex ranks of F = n - m subsets of indices into free[] (the ns - m
// unpinned positions, ascending), the "pinned rank".  For two supersets of one
// pinned set, pinned-rank order equals full-colex-rank order (colex compares
// the largest differing member first, the differing members are free ones and
// free[] is increasing), so records keep the config's full colex rank.
// C(ns - m, n - m); 0 on overflow or unless 1 <= m < n <= ns.
uint64_t pinned_total(uint32_t ns, uint32_t n, uint32_t m);
// pinned rank -> the config's n ascending positions and its full colex rank.
// `pinned`: m distinct positions < ns in any order.  False for bad sizes, a
// bad pinned list or pinned_rank >= pinned_total.
bool pinned_config(uint64_t pinned_rank, uint32_t n, uint32_t ns, const uint32_t* pinned, uint32_t m, uint32_t* out,
                   uint64_t* out_rank);

// ------------------------------------------------------------ group walk --
// Colex ranks of n-subsets sharing their n - 3 largest members form one
// contiguous "group" of C(p3, 3) ranks (bote_group.hip).  The group kernel
// runs a group in ceil(len / 64) wavefront steps plus a per-group precompute
// (group_cost: fitted), so the cost of a rank range is a sum
// over the groups it touches.  A GroupWalk holds the groups of one rank range
// [rb, re), clipped to it, in rank order.
struct GroupWalk {
  uint32_t ns = 0, n = 0, nc = 0;
  uint64_t rb = 0, re = 0;
  double group_cost = 0;
  std::vector<uint64_t> start;  // clipped group start ranks, ascending
  std::vector<uint64_t> len;    // clipped lengths (> 0)
  bool covers(uint64_t b, uint64_t e) const { return rb <= b && e <= re; }
};
// One group's precompute in wavefront steps for nc clients.
double group_cost(uint32_t nc);
// Walk the groups of [rb, re).  Null when n < 4, the range is empty or it
// touches more than max_groups groups (callers then split ranks evenly).
std::shared_ptr<GroupWalk> walk_groups(uint32_t ns, uint32_t n, uint32_t nc, uint64_t rb, uint64_t re,
                                       uint64_t max_groups = 40000000);
// nchunks + 1 ascending boundaries from b to e cutting [b, e) (inside the
// walk's range) into parts of equal estimated cost; empty if the walk does not
// cover [b, e).
std::vector<uint64_t> cut_chunks(const GroupWalk& w, uint64_t b, uint64_t e, uint32_t nchunks);
// The work-chunk table of a launch (guided): chunks of the base size
// (total / nchunks) for most of the range, then `levels` rounds of
// `tail_waves` chunks each of 1/2, 1/4, ... of it, so that the waves that
// take the last chunks finish close together.  cut_chunks when the launch
// is small (nchunks < 16 tail_waves) or tail_waves == 0.
std::vector<uint64_t> cut_chunks_guided(const GroupWalk& w, uint64_t b, uint64_t e, uint32_t nchunks,
                                        uint32_t tail_waves, uint32_t levels);
// Work chunks per wavefront for a launch of `ranks` configs on `nwaves`
// waves with nc clients: every chunk re-runs its first group's precompute
// (group_cost steps) and the launch ends about one chunk after the mean, so C
// chunks per wave cost C * g + T / C steps for T steps per wave: C = sqrt(T /
// g), between 4 and cap.  (32 per wave on a 1/64 shard of R=64 n=7 spent
// about half of its time in chunk-start precomputes.)
uint32_t chunks_per_wave(uint64_t ranks, uint32_t nwaves, uint32_t nc, uint32_t cap);
// Expected lane utilisation of the group kernel over the whole rank space.
double group_utilisation(uint32_t ns, uint32_t n);
// Group-kernel geometry choice between two workgroup sizes, each with the
// workgroups per CU (occ) and client lines per wave (gslots) it fits: true
// when (bd, occ, gslots) should replace the best so far (best_occ == 0: none).
bool pick_group_geometry(uint32_t bd, int occ, uint32_t gslots, uint32_t best_bd, int best_occ,
                         uint32_t best_gslots);

// ------------------------------------------------------------ layouts ----
// Column-major packed-u16 quad layout of `rows` (client ids) against every
// region t of an R x R matrix (row = from): entry [t][c] = lat[rows[c]][t] <<
// shift, column stride `stride` quads (quad_stride: at least one pad quad).
std::vector<uint16_t> quad_layout(const uint16_t* lat, uint32_t R, const uint32_t* rows, uint32_t nrows,
                                  uint32_t shift, uint32_t& quads, uint32_t& stride);
// Column stride in quads (8 B) for `quads` data quads: at least quads + 1,
// and an odd number of 16-B units, so that a column starts 16-B aligned
// (ds_read_b128 of two quads) and 16 lanes at consecutive columns hit 16
// distinct 4-bank groups (conflict-free 16-B reads, MI355X_MICROARCH.md LDS).
uint32_t quad_stride(uint32_t quads);
// Packed (p0 | p1 << 8 | p2 << 16) 3-subsets of [0, m) in colex order.
std::vector<uint32_t> low_table(uint32_t m);
// The fast path's preconditions (bote_sweep.hip header): every latency <=
// 4095, servers ascending, self latency 0 and server-server latency > 0 among
// the servers, >= 2 clients, and no fairness threshold.
bool fast_eligible(const uint16_t* lat, uint32_t R, const uint32_t* servers, uint32_t ns, uint32_t nc,
                   bool fairness_threshold);

// ------------------------------------------------------ sweep planning ---
// The integer arithmetic of bote_sweep_create_keys (bote_capi_sweep.hip): which
// kernel variants are exact for a planet and client count, and how often
// their narrow accumulators flush.  The C ABI copies these into FastArgs.
struct FastLimits {
  uint32_t maxlat;    // the largest latency of the planet
  uint32_t s2_flush;  // FastArgs::s2_flush, g_flush, k_flush (never 0)
  uint32_t g_flush;
  uint32_t k_flush;
  bool s32;      // FastArgs::s32: every slot's moments fit 32 bits
  bool v32;      // FastArgs::v32: s32, and every V = cnt s2 - s1^2 fits 32 bits
  bool bins_ok;  // the member bins of the group kernel cannot overflow
  bool keys32;   // bins_ok, and the extended keys' 32-bit moments are exact
};
FastLimits fast_limits(uint32_t maxlat, uint32_t nc, uint32_t n);
// (maxlat: the maximum over the R x R matrix)
FastLimits fast_limits(const uint16_t* lat, uint32_t R, uint32_t nc, uint32_t n);

// The group kernel's mean tests of compute_score (FastArgs::p_int .. m2_hi):
// p_int when both thresholds are integers, then p1i / p2i = threshold * nc;
// [lo, hi] is the band of the integer difference D in which the kernel falls
// back to the reference's f64 arithmetic (lo = hi = p * nc when p_int, else
// floor(p * nc) - 1 and ceil(p * nc) + 1), clamped to +-(2^31 - 1).
struct ScoreBands {
  int p_int;
  int64_t p1i, p2i;
  int32_t m1_lo, m1_hi, m2_lo, m2_hi;
};
ScoreBands score_bands(double p_fmean, double p_emean, uint32_t nc);

// The objective set compiled into the group kernel (DEF kernels), as
// (kind, slot) pairs: bote.py CONFIG5_OBJECTIVES, whose first
// COMPILED_OBJECTIVES_BASE entries are DEFAULT_OBJECTIVES (SCORE, MEAN af1,
// MEAN ff1, COV af1, MEAN e; then MEAN tt1, MEAN tw2, MEAN fl1).
constexpr uint32_t COMPILED_OBJECTIVES_BASE = 5, COMPILED_OBJECTIVES_KEYS = 8;
extern const uint32_t COMPILED_OBJECTIVES[COMPILED_OBJECTIVES_KEYS][2];
// True when the n_obj objectives are exactly that set: the first five on the
// base key set (keys == 0), all eight on the extended one.  A SCORE
// objective's slot is not compared.
bool is_compiled_objective_set(const uint32_t* kinds, const uint32_t* slots, uint32_t n_obj, uint32_t keys);
// Slot `slot` exists for config size n (f = 2 keys need max_f >= 2); slots
// >= 10 only with the extended key set.
bool slot_exists_n(uint32_t n, uint32_t slot, uint32_t keys);
// The values a slot's histogram holds: the n members for the colocated slots
// (5..9, 14..17), the nc Input clients for every other slot.
uint32_t slot_count(uint32_t slot, uint32_t nc, uint32_t n);

// ----------------------------------------------- percentile objectives --
// BOTE_OBJ_PCTL(bp): (kind >> 16) == 1 with the low half in 1..9999.
constexpr uint32_t PCTL_MAX_NEED = 8;  // the generic kernel's list depth
bool is_percentile_kind(uint32_t kind);
// Histogram::percentile's index (histogram.rs:110-170) for p = bp / 10000.0
// over `count` values: x = p * count in one f64 multiply (this file is built
// without contraction), idx = round(x) half away from zero, whole = (x - idx
// == 0.0).  False unless 1 <= bp <= 9999 and count >= 1.
bool percentile_index(uint32_t bp, uint32_t count, uint32_t& idx, bool& whole);
// How many of the largest values decide it: count - max(idx, 1) + 1.  The
// percentile is the need-th largest; when `whole` (idx >= 1 then), the mean of
// that one and the (need - 1)-th largest.  0 for bad arguments.
uint32_t percentile_need(uint32_t bp, uint32_t count);

// ----------------------------------------------------- MDTM objectives --
// BOTE_OBJ_MDTM's key is (H << MDTM_SUM_BITS) | S1 (include/bote_hip.h).  Both
// halves fit for every slot the library admits: at most BOTE_MAX_CLIENTS
// values of at most 2 * 16383 each, and a mean absolute deviation of at most
// half the range (2 H <= c^2 * max / 2).  S1 < 2^27 - 1, so no key is all ones.
constexpr uint32_t MDTM_SUM_BITS = BOTE_MDTM_SUM_BITS;
constexpr uint64_t MDTM_MAX_VALUE = 2 * 16383;
static_assert((uint64_t)BOTE_MAX_CLIENTS * MDTM_MAX_VALUE < (1ull << MDTM_SUM_BITS) - 1, "S1 fits its field");
static_assert((uint64_t)BOTE_MAX_CLIENTS * BOTE_MAX_CLIENTS * MDTM_MAX_VALUE / 4 < (1ull << (64 - MDTM_SUM_BITS)),
              "H fits above S1");
// H by its definition: the sum over { i : c x_i > S1 } of (c x_i - S1).
uint64_t mdtm_half_deviation(const uint32_t* x, uint32_t c);
// The key of (H, S1); false when a half does not fit its field.
bool mdtm_key(uint64_t H, uint64_t S1, uint64_t& key);

// Per start rank, the 4 u64 of FastArgs::wstate: the colex rank of the
// config's n - 3 largest positions (its group: the config with its three
// lowest positions zeroed), then those positions as bytes in two words (n - 3
// <= 16), then 0.  False when a rank is out of range.
bool chunk_states(const uint64_t* starts, uint32_t count, uint32_t n, uint32_t ns, std::vector<uint64_t>& out);
// The sample launch of the top-K seed over [rb, re) of `total` ranks, on
// nwaves waves, for the K least: the number of one-step (64-config) sample
// chunks, 0 when the range is too small to sample.
uint32_t sample_count(uint64_t rb, uint64_t re, uint64_t total, uint32_t nwaves, uint32_t K);
// Their start ranks: evenly spaced over [rb, re - 64].
std::vector<uint64_t> sample_starts(uint64_t rb, uint64_t re, uint32_t nsamp);
// Consecutive ranks per lane job of the fast and generic kernels: 1 to 32, so
// that a launch of `count` ranks has ~8 jobs per lane on grid x bd lanes.
uint32_t sweep_runlen(uint64_t count, uint32_t grid, uint32_t bd);

// -------------------------------------------------------- result blocks --
// A result block is [n_obj x kp records {key, rank} (16 B), ascending, padded
// with all-ones records][valid u64][digest u64].  Copies the first K records
// of each objective to out (n_obj x K, padding past the filled ones).
struct TopkRecord {
  uint64_t key, rank;
};
void unpack_result(const uint8_t* blk, uint32_t n_obj, uint32_t K, uint32_t kp, TopkRecord* out, uint32_t* out_count,
                   uint64_t* out_valid, uint64_t* out_digest);

// ------------------------------------------------------ argument checks --
// What the C ABI (bote_capi*.hip) refuses before it touches a device: a
// BOTE_E_* code and the text bote_last_error() then returns.  Each function
// applies its checks in a fixed order and reports the first that fails; the
// per-entry functions are the whole sequence of one entry point after its
// null-handle test.  They take the planet's region count R, not the handle;
// R == 0 stands for a null planet ("planet is null").
struct Status {
  int code = BOTE_OK;
  std::string msg;
};
// `n` region ids below R (null only when n == 0), optionally pairwise distinct.
Status check_regions(const uint32_t* ids, uint32_t n, uint32_t R, bool distinct, const char* what);
// Distinct ids among `n` checked ones.
uint32_t distinct_count(const uint32_t* ids, uint32_t n, uint32_t R);
// ncfg explicit configs of n positions: each below ns, none twice in a config.
// Needs ns <= 256 (the entries check the server list first: ns <= R <= 128).
Status check_configs(const uint32_t* configs, uint64_t ncfg, uint32_t n, uint32_t ns);
// [rank_begin, rank_begin + ncfg) inside the C(ns, n) ranks.
Status check_rank_range(uint32_t ns, uint32_t n, uint64_t rank_begin, uint64_t ncfg);
// rank_begin <= rank_end <= C(ns, n).
Status check_rank_span(uint32_t ns, uint32_t n, uint64_t rank_begin, uint64_t rank_end);
Status check_ft_metric(int ft_metric);
// A search over n-subsets of the server list: the planet, min_n <= n <= 16
// (min_n = 2: FPaxos needs q = 2; 1: leaderless quorums only; no other value
// is meant: it picks between the two entries' texts), n <= ns, nc <= 4096,
// then distinct servers and clients below R.
Status check_search_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                         uint32_t n, uint32_t min_n);
// bote_quorum_latencies .. bote_all_leaders (mode: bote::launch_single's; 2 reads `leader`).
Status check_single_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                         const uint32_t* froms, uint32_t nf, uint32_t q, uint32_t leader, int mode);
Status check_best_leader_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                              uint32_t q, int stat);
// bote_eval and bote_eval_keys (configs null: the rank range).
Status check_eval_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                       uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg,
                       const bote_ranking_params* rp, uint32_t keys);
Status check_leaderless_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                             uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg,
                             const uint32_t* quorum_sizes, uint32_t nq);
// bote_sweep_create_keys; has_score: some objective is BOTE_OBJ_SCORE.  In
// order: the key set, the kernel path, check_search_args, the objective
// count, a null list, K, then per objective its kind, slot range and slot
// existence for n and, for a percentile, that it needs at most PCTL_MAX_NEED
// of the slot's largest values; then a MAX objective on a forced group kernel
// (which does not compute it), a percentile objective on one, SCORE without
// ranking params, and the ft_metric.
Status check_sweep_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                        uint32_t n, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                        const bote_ranking_params* rp, int kernel, uint32_t keys, bool& has_score);
// bote_sweep_create_constrained, after check_sweep_args.  In order: a null list
// with n_con > 0; then per constraint an unknown kind, the SCORE kind (not a
// constraint), its slot's range and existence for n and, for a percentile, the
// PCTL_MAX_NEED values (BOTE_E_RANGE, as for objectives); then n_obj + n_con
// above BOTE_MAX_OBJECTIVES (BOTE_E_RANGE); then, with n_con > 0, the extended
// key set and a forced group kernel (neither applies constraints).
Status check_constraint_args(uint32_t nc, uint32_t n, const bote_constraint* cons, uint32_t n_con, uint32_t n_obj,
                             int kernel, uint32_t keys);
// The fast kernel's variant for a sweep's key entries, its objectives and its
// constraints alike (kinds as the kernels take them, a percentile with its need:
// bote_kernels.hpp OBJ_PCTL): a MAX entry means maxima (TAIL_MAX), a percentile
// lists (TAIL_LIST, which serve a MAX too; `need` is the deepest one's), an MDTM
// entry the MDTM variant (TAIL_MDTM), which carries neither: `mixed` when it
// stands beside a MAX or a percentile (the generic kernel then).  The values
// are bote::FAST_*.
enum { TAIL_PLAIN = 0, TAIL_MAX = 1, TAIL_LIST = 2, TAIL_MDTM = 3 };
constexpr uint32_t DEV_KIND_PCTL = 0x10000u, DEV_PCTL_NEED_MASK = 15u;
struct TailPlan {
  int tail = TAIL_PLAIN;
  uint32_t need = 0;
  bool mixed = false;
};
TailPlan fast_tail_plan(const uint32_t* dev_kinds, uint32_t n_keys);
// bote_sweep_create_pinned, after check_sweep_args.  In order: a null or empty
// pinned list, n_pinned >= n, a position >= ns, a repeated position, a forced
// group kernel (it does not sweep pinned members), the extended key set (the
// entry takes none: the internal path only).
Status check_pinned_args(uint32_t ns, uint32_t n, const uint32_t* pinned, uint32_t n_pinned, int kernel,
                         uint32_t keys);
// bote_batch_create, after check_sweep_args; check_pinned_args on set 0 follows
// it (a forced group kernel, with the pinned sweep's text).  In order: the set
// count (1 .. BATCH_MAX_SETS), a null list or m outside 1 .. n - 1, then per
// set, lowest index first, a position >= ns and a repeated position, each
// naming the set; then the extended key set.
constexpr uint32_t BATCH_MAX_SETS = BOTE_BATCH_MAX_SETS;
Status check_batch_args(uint32_t ns, uint32_t n, const uint32_t* pinned, uint32_t n_sets, uint32_t m, uint32_t keys);
// The unit plan of a batch (DESIGN.md §4 "Batched pinned sweeps"): every set's
// C(ns - m, n - m) pinned ranks are cut into the same `slices` slices, slice s
// being [bounds[s], bounds[s + 1]), and a unit is (set, slice): units = B *
// slices.  One slice when a set fits one pass of a workgroup (BATCH_PASS
// configs); otherwise as many as fill the grid (`grid_cap` workgroups; 0: no
// cap, as many as there are), at most BATCH_MAX_SLICES, so that the slices'
// lists and the set's fix-up list are one 8-way merge group.  `runlen`: the
// consecutive ranks of a lane job.  slices == 0: bad sizes.
constexpr uint32_t BATCH_MAX_SLICES = 7, BATCH_PASS = 8192, BATCH_LANES = 256;
struct BatchPlan {
  uint32_t slices = 0;
  uint64_t total = 0, slice_len = 0;
  std::vector<uint64_t> bounds;  // slices + 1
  uint64_t units = 0;
  uint32_t runlen = 0;
};
BatchPlan batch_plan(uint32_t ns, uint32_t n, uint32_t m, uint32_t n_sets, uint32_t grid_cap);
// ----------------------------------------------------- bounded batches --
// The reference's filter between two levels of an evolving chain
// (Search::min_mean_decrease, search.rs:403-419; DESIGN.md §4 "Streaming
// evolving search"): for f in FTMetric::fs(n - 2), on the Atlas f Input slot,
//   fl(prev_s1 / count) - fl(s1 / count) >= min_mean_decrease
// (Histogram::mean_improv: two rounded divisions, one rounded subtraction).
// fl(s1 / count) is non-decreasing in s1 and the rounded difference
// non-increasing in its subtrahend, so the passing sums are exactly s1 < limit.
// MEAN_SUM_END: every S1 the library admits is below it (4096 clients of at
// most 2 * 16383); MEAN_NO_BOUND: the kernels' "no bound" (PinArgs::lim).
constexpr uint64_t MEAN_SUM_END = 1ull << BOTE_MDTM_SUM_BITS;
constexpr uint32_t MEAN_NO_BOUND = 0xFFFFFFFFu;
static_assert((uint64_t)BOTE_MAX_CLIENTS * 2 * 16383 < MEAN_SUM_END, "every S1 is below the search range's end");
// The predicate itself, each step one rounded f64 operation (count >= 1).
bool mean_decrease_passes(uint64_t prev_s1, uint64_t s1, uint32_t count, double min_mean_decrease);
// The least s1 in [0, MEAN_SUM_END] that does not pass (MEAN_SUM_END: all
// pass; 0: none does, a NaN threshold among the reasons), by binary search.
uint32_t mean_decrease_limit(uint64_t prev_s1, uint32_t count, double min_mean_decrease);
// A set's two limits (SLOT_AF1, SLOT_AF2) for configs of size n from its
// previous level's sums prev_s1[0..1]: MEAN_NO_BOUND where f is not in fs(n - 2).
void batch_limits(const uint64_t* prev_s1, uint32_t n, uint32_t nc, double min_mean_decrease, int ft_metric,
                  uint32_t* out_lim);
// bote_mean_decrease_limit: a null out, count 0, a sum >= MEAN_SUM_END.
Status check_mean_limit_args(uint64_t prev_s1, uint32_t count, const uint32_t* out_limit);
// bote_batch_create_bounded, after bote_batch_create's checks.  In order: null
// ranking params, a null prev_s1, no clients, then per set, lowest index first,
// a sum >= MEAN_SUM_END, naming the set.
Status check_bounded_args(const uint64_t* prev_s1, uint32_t n_sets, uint32_t nc, const bote_ranking_params* rp);
// rank_begin <= rank_end <= `total` (a pinned sweep's pinned_total).
Status check_rank_span_total(uint64_t total, uint64_t rank_begin, uint64_t rank_end);
// ------------------------------------------------------- census sweeps --
// (DESIGN.md §4 "Census sweeps": counts of the configs ranked before given records)
constexpr uint32_t CENSUS_MAX_THRESHOLDS = BOTE_CENSUS_MAX_THRESHOLDS;
// bote_census_create.  In order: a forced group kernel (it is not touched by
// censuses), then check_sweep_args with K = 1 on the base key set.
Status check_census_args(uint32_t R, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                         uint32_t n, const bote_objective* objs, uint32_t n_obj, const bote_ranking_params* rp,
                         int kernel, bool& has_score);
// The kernel a census runs (path: 0 generic, 1 fast), as pinned sweeps are
// routed.  `eligible`: fast_eligible's verdict on the planet and lists.  AUTO
// and a forced fast kernel run the fast kernel's census variant on an eligible
// planet with only SCORE, MEAN and COV objectives; a MAX, percentile or MDTM
// objective, an ineligible planet and a forced generic kernel run the generic
// kernel's; a forced fast kernel with such an objective, or on an ineligible
// planet, is BOTE_E_ARG.
Status census_route(bool eligible, const bote_objective* objs, uint32_t n_obj, int kernel, int& path);
// bote_census_launch.  In order: T outside 1 .. CENSUS_MAX_THRESHOLDS, a null
// list, then per objective, lowest index first, a threshold below its
// predecessor in the unsigned (key, rank) order (equal neighbours pass; any u64
// is a legal key), then the rank span.
Status check_census_launch(const TopkRecord* thr, uint32_t n_obj, uint32_t T, uint32_t ns, uint32_t n,
                           uint64_t rank_begin, uint64_t rank_end);

// bote_evolving_chains' six levels (n = 3, 5, .., 13): arrays present where a
// level has entries, every mask an n-subset of the ns servers.
Status check_chain_levels(uint32_t ns, const uint32_t* counts, const uint64_t* const* masks,
                          const double* const* scores, const double* const* means);

}  // namespace host
}  // namespace bote
