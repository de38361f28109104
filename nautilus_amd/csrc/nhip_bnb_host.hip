// nhip_bnb_host.hip -- host side of the branch-and-bound matcher (nhip_bnb.hip holds the kernels).  bnb_plan decides the
// form a pair list takes and is the only reader of the NHIP_BNB_* test hooks; launch_csm_bnb carries a plan out: the
// kernels' parameters, the instrumentation's buffers, the workspace's layout, the helper streams of the overlapped rounds.
// Every form returns the same records; tests run them all (NHIP_TUNABLES=1 lets a process choose the form per launch).
#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "nhip_bnb_params.h"

namespace nhip {

using namespace bnb;

namespace {

size_t bnb_lds_first(const GridLayout &L, bool pool_lds) {
  const size_t pool = pool_lds ? (size_t)L.pool_bytes : 0;
  return pool > (size_t)ORG_LDS ? pool : (size_t)ORG_LDS;
}
size_t bnb_lds_bytes(const GridLayout &L, const nhip_search_t *search, bool pool_lds) {
  // (the fused form's size; the split form's is no larger: nhip_bnb_params.h)
  return lds_bytes(bnb_lds_first(L, pool_lds), search->n_theta, false);
}
constexpr size_t LDS_MAX = 160 * 1024;

struct TimerScope {  // (an error return between timer_begin and timer_end closes the open slot)
  int id;
  hipStream_t s;
  TimerScope(int i, hipStream_t st) : id(i), s(st) { timer_begin(id, s); }
  ~TimerScope() { timer_end(id, s); }
};
}  // namespace

bool bnb_fits(const GridLayout &L, const nhip_search_t *search) {
  const int nbx = (search->nx + BNB_B - 1) / BNB_B, nby = (search->ny + BNB_B - 1) / BNB_B;
  // (the pooled table goes to LDS when it fits beside the bounds; else it is read from global memory)
  return nbx <= NB && nby <= NB && bnb_lds_bytes(L, search, false) <= LDS_MAX && L.pool_bytes % 16 == 0 &&
         L.pool_bytes < (1ll << RUN_SHIFT) && L.S + 2 * L.pad < 65536 && search->n_theta <= MAX_ROT;
}

// Instrumentation buffers (NHIP_BNB_INSTRUMENT=1 only): process-wide, allocated on first use, guarded by g_instr_mu
static std::mutex g_instr_mu;
static unsigned long long *g_bnb_timeline = nullptr;
static unsigned long long *g_bnb_stats = nullptr;

constexpr int64_t BNB_WS_HEADER = 256;  // per XCD 32 bytes: {entries filled, next entry to work}
// Lists of fewer than SPLIT_MIN_PAIRS pairs: room for 16 handed-over rotations per pair on average (what does not fit is
// worked by the pair's own workgroup).  The split form: per pair its four counters, 1.5 entries of the candidates' work
// list and the rows of bounds of up to 64 rotations.  Lists of SPLIT_MIN_PAIRS .. SPLIT_PAIRS pairs take it in ONE round;
// longer lists in rounds of SPLIT_PAIRS with the candidates of a round on a helper stream beside the next round's bounds,
// which needs two rounds' state (8.6 GB at 61 rotations); with less workspace they stay fused.  Measured (match ms,
// one kernel per pair + hand-over / split; tools/r04_small_lists.sh, profiles/r04_small_lists.txt): 30 pairs 0.21 / 0.21,
// 100 pairs 0.23 / 0.28, 200 pairs 0.71 / 0.60, 300 pairs 1.09 / 0.79, 500 pairs 1.12 / 0.86, 1,000 pairs 1.60 / 1.21,
// 2,000 pairs 4.02 / 1.95, 3,000 pairs 4.08 / 2.63 (round 3's per-XCD work lists: 4.70), 10,000 pairs 8.1 / 6.4; round 3,
// 40,000 pairs 27.1 / 22.8, 1,000,000 pairs at 100 per target 606 fused, 663 in rounds of 65,536 without the helper
// stream (every round pays its own tail), 600 with it, 543 in rounds of 131,072 with it.
constexpr int64_t SPLIT_PAIRS = 131072, SPLIT_MIN_PAIRS = 192, SPLIT_RING = 16;
// Rounds of fewer pairs than this deal the additional workgroups of their heavy pairs over all eight XCDs' lists
// (csm_bnb_order_spread_kernel); longer ones keep them in the pair's home list (csm_bnb_order_kernel), where every XCD
// has heavy pairs of its own and the tables stay L2-resident.  Measured, match ms home / spread: 3,000 pairs 4.70 / 2.63,
// 4,500 pairs 3.39 / 3.46, 10,000 pairs 6.38 / 6.54 (profiles/r04_small_lists.txt).
constexpr int64_t SPREAD_BELOW_PAIRS = 4096;
constexpr int64_t SPLIT_SLOT_FIXED = 8 * 64 * 4 + 1024;  // per batch: the work lists' floor of 64 extra entries, alignment
// Pairs with at least 64 candidates left (a quarter of a configs[1] list, most of its work) go to the front of their
// XCD's list: profiles/r06_front_min.txt -- 0 / 40 / 70 / 100 / 150: 3.01 / 2.90 / 2.87 / 2.92 / 2.96 ms per 10,000 pairs
constexpr uint32_t FRONT_MIN = 64;

// The split form's state of `pairs` pairs at n_theta rotations in `batches` rounds: the size rule and the slots price it.
static int64_t split_state_bytes(int64_t pairs, int64_t batches, int32_t n_theta) {
  return batches * SPLIT_SLOT_FIXED + pairs * (16 + 6 + (int64_t)n_theta * 512);
}
// Workgroups per pair at most in a round of nb pairs (no NHIP_BNB_SPLIT_MAX).  With the heavy pairs at the front of the
// list -- FRONT_MIN -- their workgroups start with the launch, and rounds of 8,192 pairs and more are long enough for four
// of them to finish the heaviest pair inside it: 8 / 6 / 5 / 4 / 3 per pair measured 2.87 / 2.84 / 2.80 / 2.79 / 2.94 ms
// on configs[1], 16-bit cells, 2.86 / 3.00 / 2.79 / 2.72 / 2.79 with 8-bit cells: profiles/r06_front_min.txt.
static uint32_t bnb_split_max(int64_t nb) { return nb < SPREAD_BELOW_PAIRS ? 16u : (nb >= 8192 ? 4u : 8u); }

int64_t bnb_workspace_bytes_lists(int32_t n_pairs) {  // (the hand-over lists alone: the one-kernel form)
  const int64_t n = n_pairs > 0 ? n_pairs : 0;
  return BNB_WS_HEADER + 8 * (((n + 7) / 8) * 16 + 64) * (int64_t)sizeof(RotEntry);
}
int64_t bnb_workspace_bytes(int32_t n_pairs) {
  const int64_t n = n_pairs > 0 ? n_pairs : 0;
  // (whether a list is sized for the split form depends on its length and the hooks alone: the plan of any lattice says)
  nhip_search_t any = {};
  const int64_t m = n <= SPLIT_PAIRS ? n : 2 * SPLIT_PAIRS;  // (a longer list: two rounds' state, for the helper stream)
  const int64_t split = bnb_plan(GridLayout(), &any, (int32_t)n, 0).sized_split
                            ? BNB_WS_HEADER + split_state_bytes(m, m / 512 + 4, 64) : 0;
  return std::max(bnb_workspace_bytes_lists(n_pairs), split);
}

BnbPlan bnb_plan(const GridLayout &L, const nhip_search_t *search, int32_t n_pairs, int64_t workspace_bytes) {
  const auto is = [](const char *v, char c) { return v && v[0] == c; };
  const auto num = [](const char *name, int unset) { const char *v = tunable(name); return v ? atoi(v) : unset; };
  const char *force = tunable("NHIP_BNB_KERNELS");      // 1: never hand over, 2: always
  const char *sp = tunable("NHIP_BNB_SPLIT");           // 0: never the split form, 1: whenever the workspace allows
  const char *sbat = tunable("NHIP_BNB_SPLIT_BATCH");   // <pairs> per round
  const char *smax = tunable("NHIP_BNB_SPLIT_MAX");     // <workgroups per pair>
  BnbPlan p = {};
  p.n_pairs = n_pairs;
  p.cb = L.cb;
  p.levels = is(tunable("NHIP_BNB_LEVELS"), '1') ? 1 : 2;  // (1: without the sub-block bounds)
  p.l2_runs = !is(tunable("NHIP_BNB_L2_RUNS"), '0');       // (0: strip bounds per stored cell everywhere -- the A/B, tests)
  p.pair_subs = !is(tunable("NHIP_BNB_PAIR_SUBS"), '0');   // (0: one pass of exact sums per sub-block -- the A/B, tests)
  p.zero_chunks = !is(tunable("NHIP_BNB_ZERO_CHUNKS"), '0');  // (0: the exact sums visit every chunk of the cell list -- the A/B, tests)
  p.seed_bounds = is(tunable("NHIP_BNB_SEED_BOUNDS"), '1');  // (1: the seeds take their sub-block bounds while the best sum is 0 too -- the A/B, tests)
  p.general_all = is(tunable("NHIP_BNB_QUEUE"), '1');      // (the general path for every scan)
  static_assert(NHIP_SHORT_SCAN_POINTS == 64 * OCL, "the header's promise is the by-rotation form's limit");
  p.short_scans = (search->flags & NHIP_SEARCH_SHORT_SCANS) != 0 && !p.general_all && (uint32_t)(L.S + 2 * L.pad) < ORG_LIMIT;
  p.instrumented = is(tunable("NHIP_BNB_INSTRUMENT"), '1');
  p.stats = p.instrumented && is(tunable("NHIP_BNB_STATS"), '1');
  p.timeline = p.instrumented && is(tunable("NHIP_BNB_TIMELINE"), '1');
  p.sized_split = n_pairs >= SPLIT_MIN_PAIRS || (n_pairs > 0 && (is(sp, '1') || sbat));
  // The split form's rounds as the workspace allows them; the hand-over lists only for lists that do not take it.
  if (workspace_bytes > 0 && n_pairs > 0 && !p.general_all && !is(sp, '0') && !is(force, '2') &&
      (n_pairs >= SPLIT_MIN_PAIRS || is(sp, '1'))) {
    p.batch = sbat && atoi(sbat) > 0 ? atoi(sbat) : SPLIT_PAIRS;
    if (p.batch > n_pairs) p.batch = n_pairs;
    for (;;) {  // (a workspace too small for two batches in flight: smaller batches, down to 512 pairs)
      p.slot_bytes = (split_state_bytes(p.batch, 1, search->n_theta) + 511) & ~(int64_t)511;
      p.slots = (workspace_bytes - BNB_WS_HEADER - 512) / p.slot_bytes;
      const int64_t rounds = (n_pairs + p.batch - 1) / p.batch;
      if (p.slots >= (rounds < 2 ? rounds : 2) || p.batch <= 512) break;
      p.batch = p.batch / 2 > 512 ? p.batch / 2 : 512;
    }
    if (p.slots > SPLIT_RING) p.slots = SPLIT_RING;
    if (p.slots < 1) p.batch = 0;  // (no room: the fused form)
    // (several rounds pay off only with the helper stream, i.e. with two rounds' state, and in rounds that are long)
    if (!sbat && p.batch > 0 && n_pairs > p.batch && (p.slots < 2 || p.batch < SPLIT_PAIRS)) p.batch = 0;
  }
  p.rounds = p.batch > 0 ? (n_pairs + p.batch - 1) / p.batch : 1;
  if (p.batch > 0)
    p.form = !is(tunable("NHIP_BNB_SPLIT_OVERLAP"), '0') && p.slots >= 2 && n_pairs > p.batch
                 ? BNB_SPLIT_OVERLAP : (p.rounds > 1 ? BNB_SPLIT_ROUNDS : BNB_SPLIT_ONE);
  p.split_min = (uint32_t)std::max(num("NHIP_BNB_SPLIT_MIN", 300), 1);  // <candidates per additional workgroup of a pair>
  p.split_max = smax ? (uint32_t)std::max(atoi(smax), 1) : 0u;
  // Work sharing.  A flat landscape leaves a pair thousands of candidates (the median pair: ~30): alone on the
  // chip its workgroup is busy for 3 ms (the median pair: 0.2 ms), and a batch that does not fill the chip many
  // times over waits for it.  Such a pair (>= heavy_min candidates after bounds and seeds) works only its first
  // keep_ranks rotations in best-first order (one per wave) itself and hands the others, with the masks of their
  // candidate blocks, to per-XCD lists in the caller's workspace; a second kernel works the lists with every wave of
  // the chip, sharing the pair's running best through keys[pair].  Measured (tools/bnb_heavy.py, bnb_quick.py;
  // profiles/r02_bnb_heavy.json): the heaviest pair alone 2.2 -> 0.94 ms; 30 pairs 0.80 -> 0.45 ms; 500 pairs + the
  // three heaviest 2.5 -> 1.3 ms.  From ~1000 pairs on the chip is full anyway and handing over only loses pruning
  // and L2 locality (2,000 pairs 4.6 -> 7.3 ms, 10,000 pairs unchanged), so large batches do not.  (Also tried:
  // letting the waves of finished workgroups take entries inside the first kernel, and persistent workgroups -- never
  // a gain.)  Lists that take the split form do not hand rotations over: their candidates' launch shares the heavy
  // pairs among several workgroups.
  p.heavy_min = (uint32_t)num("NHIP_BNB_HEAVY_MIN", n_pairs <= 64 ? 1 : 384);
  p.keep_ranks = (uint32_t)num("NHIP_BNB_KEEP_RANKS", 8);
  // (a pair keeps its first keep_ranks rotations: a search of no more rotations than that -- the seven per workgroup of
  //  GetTransformation's fine level -- can hand nothing over, and the second kernel's launch, 22 us of a 230 us call, is left out)
  const bool second = force ? force[0] == '2' : (n_pairs < 1024 && p.batch == 0 && (uint32_t)search->n_theta > p.keep_ranks);
  p.second = second && !p.general_all && workspace_bytes >= BNB_WS_HEADER + 8 * (int64_t)sizeof(RotEntry);
  if (p.second)  // (entries per XCD list)
    p.rot_cap = (uint32_t)std::min<int64_t>((workspace_bytes - BNB_WS_HEADER) / (int64_t)sizeof(RotEntry) / 8, 0x0fffffff);
  p.pool_lds = bnb_lds_bytes(L, search, true) <= LDS_MAX;
  p.lds_first = (int64_t)bnb_lds_first(L, p.pool_lds);
  return p;
}

// The helper stream of the split form (the candidates of round i run beside the bounds of round i + 1) and the events
// that order the two.  One set per CALL IN FLIGHT, taken from a per-device pool: a host with one thread per device
// (nhip_set_device) gets a stream and events of ITS device, and two threads on one device never share
// events -- a wait binds to the event's latest record, so a shared ring would let one caller's candidates start on the
// other's bounds.  The pool's mutex is held only to take a set and to put it back, never across the enqueue: the set
// goes back as soon as the call has enqueued its work (the waits already issued stay bound to their records, and the
// helper stream runs in order, so the next user queues up behind).  Sets live until the process ends.
struct SplitSet {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ea[SPLIT_RING], eb[SPLIT_RING];
};
static std::mutex g_split_mu;
static std::vector<SplitSet *> g_split_free;

static int split_set_acquire(SplitSet **out) {
  int dev = -1;
  NHIP_TRY_HIP(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lock(g_split_mu);
    for (size_t i = 0; i < g_split_free.size(); i++)
      if (g_split_free[i]->device == dev) {
        *out = g_split_free[i];
        g_split_free.erase(g_split_free.begin() + (long)i);
        return NHIP_OK;
      }
  }
  SplitSet *n = new SplitSet();
  n->device = dev;
  hipError_t e = hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking);
  for (int i = 0; i < SPLIT_RING && e == hipSuccess; i++) {
    e = hipEventCreateWithFlags(&n->ea[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&n->eb[i], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    delete n;  // (what was created stays with the runtime: an allocation failure of streams / events is not a path to tidy)
    return hip_fail(e, "split form: helper stream / events", __FILE__, __LINE__);
  }
  *out = n;
  return NHIP_OK;
}
static void split_set_release(SplitSet *set) {
  if (!set) return;
  std::lock_guard<std::mutex> lock(g_split_mu);
  g_split_free.push_back(set);
}

// What the calling thread's last launch_csm_bnb did (nhip_csm_last_launch: tests assert the form a list took).
static thread_local BnbPlan t_last_plan = {};
void bnb_last_launch(int32_t out[8]) {
  const BnbPlan &p = t_last_plan;
  const int32_t info[8] = {p.form, (int32_t)p.batch, (int32_t)p.slots, (int32_t)p.rounds, p.short_scans, p.second,
                           (int32_t)p.instrumented | ((int32_t)p.l2_runs << 1) | ((int32_t)p.pair_subs << 2) |
                               ((int32_t)p.zero_chunks << 3) | ((int32_t)p.seed_bounds << 4), p.n_pairs};
  memcpy(out, info, sizeof(info));
}

// The kernels' parameters: the job's, then what follows from the layout and the plan
static void fill_bnb_params(BnbParams &P, const MatchJob &job, const BnbPlan &plan) {
  const GridLayout &L = *job.L;
  fill_job_params(P, job);
  P.pair_kbase = job.pair_kbase;
  P.keys = reinterpret_cast<unsigned long long *>(job.keys);
  P.gate = job_gate(job);  // (a kernel parameter only: the plan does not read it)
  P.nbx = (P.nx + BNB_B - 1) / BNB_B;
  P.nby = (P.ny + BNB_B - 1) / BNB_B;
  P.pool_pitch = L.pool_pitch;
  P.pool_rows = L.pool_rows;
  P.pairs_per_xcd = (plan.n_pairs + 7) / 8;
  P.skip_bytes = L.skip_bytes;
  P.pool_bytes = L.pool_bytes;
  P.pool4_bytes = L.pool4_bytes;
  P.pool4_pitch = L.pool4_pitch;
  P.hi_offset = L.hi_offset;
  P.hi_bytes = L.hi_bytes;
  P.hi_pitch = L.hi_pitch;
  P.hi_tpr = L.hi_tpr;
  P.hi_copy_bytes = L.hi_copy_bytes;
  P.t16_bytes = L.t16_bytes;
  P.t16_tpr = L.t16_tpr;
  P.inv_res_f = (float)P.inv_res;
  P.levels = plan.levels;
  P.l2_runs = plan.l2_runs;
  P.pair_subs = plan.pair_subs;
  P.zero_chunks = plan.zero_chunks;
  P.seed_bounds = plan.seed_bounds;
  P.general_all = plan.general_all;
  P.short_scans = plan.short_scans;
  P.heavy_min = plan.heavy_min;
  P.keep_ranks = plan.keep_ranks;
  P.rot_cap = plan.rot_cap;
  P.lds_first = (int32_t)plan.lds_first;
}

// The instrumented build's counters and timestamps, as the plan asks for them
static int instr_buffers(const BnbPlan &plan, BnbParams &P, hipStream_t s) {
  if (!plan.stats && !plan.timeline) return NHIP_OK;
  std::lock_guard<std::mutex> lock(g_instr_mu);
  if (plan.stats) {
    if (!g_bnb_stats) {
      NHIP_TRY_HIP(hipMalloc(reinterpret_cast<void **>(&g_bnb_stats), 8 * (BNB_STATS_HEAD + (size_t)BNB_STATS_PAIRS + BNB_STATS_CHUNKS + BNB_STATS_SEEDS)));
      NHIP_TRY_HIP(hipMemset(g_bnb_stats, 0, 8 * (BNB_STATS_HEAD + (size_t)BNB_STATS_PAIRS + BNB_STATS_CHUNKS + BNB_STATS_SEEDS)));
    }
    P.stats = g_bnb_stats;
  }
  if (plan.timeline) {
    if (!g_bnb_timeline) NHIP_TRY_HIP(hipMalloc(reinterpret_cast<void **>(&g_bnb_timeline), 48 * (size_t)BNB_STATS_PAIRS + 16));
    P.timeline = g_bnb_timeline;
    // (the candidates' launch of the split form: first start / last end per pair)
    NHIP_TRY_HIP(hipMemsetAsync(g_bnb_timeline + 4 * (size_t)BNB_STATS_PAIRS + 2, 0xff, 8 * (size_t)BNB_STATS_PAIRS, s));
    NHIP_TRY_HIP(hipMemsetAsync(g_bnb_timeline + 5 * (size_t)BNB_STATS_PAIRS + 2, 0, 8 * (size_t)BNB_STATS_PAIRS, s));
    const unsigned long long init[2] = {~0ull, 0ull};  // the second kernel's first start and last end
    NHIP_TRY_HIP(hipMemcpyAsync(g_bnb_timeline + 4 * (size_t)BNB_STATS_PAIRS, init, 16, hipMemcpyHostToDevice, s));
  }
  return NHIP_OK;
}

// The split form, round by round.  Candidates (bound by the L1's lookups) beside the next batch's bounds (bound by the
// vector ALUs): the first part of every batch on the caller's stream, the second on the helper stream (BNB_SPLIT_OVERLAP;
// else on the caller's stream too), each batch's state in its own slot of the workspace.
static int run_rounds(const BnbParams &P, const BnbPlan &plan, const BnbLaunchers &K, void *d_workspace,
                      int64_t workspace_bytes, hipStream_t s) {
  const bool overlap = plan.form == BNB_SPLIT_OVERLAP;
  SplitSet *set = nullptr;
  if (overlap) {
    const int rc = split_set_acquire(&set);
    if (rc) return rc;
  }
  std::unique_ptr<SplitSet, void (*)(SplitSet *)> set_guard(set, split_set_release);
  hipStream_t s2 = overlap ? set->stream : s;
  uint8_t *base = static_cast<uint8_t *>(d_workspace) + BNB_WS_HEADER;
  base += (512 - (reinterpret_cast<uintptr_t>(base) & 511)) & 511;
  int64_t round = 0;
  for (int64_t b0 = 0; b0 < plan.n_pairs; b0 += plan.batch, round++) {
    const int32_t nb = (int32_t)(plan.n_pairs - b0 < plan.batch ? plan.n_pairs - b0 : plan.batch);
    BnbParams Q = P;
    Q.pair_src += b0;
    Q.pair_slot += b0;
    Q.rot0_cs += 2 * b0;
    if (Q.pair_origin) Q.pair_origin += 2 * b0;
    Q.keys += b0;
    Q.pair_base = (int32_t)b0;  // (what nhip_dev_status names is an index into the CALLER's arrays)
    Q.n_pairs = nb;
    Q.pairs_per_xcd = (nb + 7) / 8;
    Q.ps_work_stride = Q.pairs_per_xcd + (Q.pairs_per_xcd / 2 > 64 ? Q.pairs_per_xcd / 2 : 64);
    Q.split_min = plan.split_min;
    Q.split_max = plan.split_max ? plan.split_max : bnb_split_max(nb);
    Q.front_min = FRONT_MIN;
    uint8_t *w = base + (round % plan.slots) * plan.slot_bytes;
    Q.ps_count = reinterpret_cast<uint32_t *>(w);
    Q.ps_live = Q.ps_count + nb;
    Q.ps_next = Q.ps_live + nb;
    Q.ps_nw = Q.ps_next + nb;
    // (spread form: the ticket counter of the additional workgroups, zeroed with the four arrays before it)
    const bool spread = nb < SPREAD_BELOW_PAIRS;
    Q.ps_ticket = spread ? Q.ps_nw + nb : nullptr;
    Q.ps_work = reinterpret_cast<int32_t *>(Q.ps_nw + nb + 4);
    const uintptr_t rows = (reinterpret_cast<uintptr_t>(Q.ps_work + 8 * (size_t)Q.ps_work_stride) + 511) & ~(uintptr_t)511;
    Q.ps_rows = reinterpret_cast<uint32_t *>(rows);
    NHIP_REQUIRE((int64_t)(rows - reinterpret_cast<uintptr_t>(w)) + (int64_t)nb * P.n_theta * 512 <= plan.slot_bytes &&
                     w + plan.slot_bytes <= static_cast<uint8_t *>(d_workspace) + workspace_bytes,
                 "csm_bnb: workspace accounting");
    // (the slot's previous batch must be through its candidates)
    if (overlap && round >= plan.slots) NHIP_TRY_HIP(hipStreamWaitEvent(s, set->eb[(round - plan.slots) % SPLIT_RING], 0));
    NHIP_TRY_HIP(hipMemsetAsync(w, 0, 16 * (size_t)nb + 16, s));
    if (spread) NHIP_TRY_HIP(hipMemsetAsync(Q.ps_work, 0xff, 32 * (size_t)Q.ps_work_stride, s));  // (-1: no pair)
    {
      TimerScope t_a(NHIP_TIMER_CSM_BOUNDS, s);
      const int rc = K.split_a(Q, plan, s);
      if (rc) return rc;
    }
    if (overlap) {
      NHIP_TRY_HIP(hipEventRecord(set->ea[round % SPLIT_RING], s));
      NHIP_TRY_HIP(hipStreamWaitEvent(s2, set->ea[round % SPLIT_RING], 0));
    }
    {
      TimerScope t_b(NHIP_TIMER_CSM_CAND, s2);
      const int rc = K.split_b(Q, plan, s2);
      if (rc) return rc;
    }
    if (overlap) NHIP_TRY_HIP(hipEventRecord(set->eb[round % SPLIT_RING], s2));
  }
  // (the helper stream works in order: its last batch done, all are)
  if (overlap) NHIP_TRY_HIP(hipStreamWaitEvent(s, set->eb[(round - 1) % SPLIT_RING], 0));
  return NHIP_OK;
}

int launch_csm_bnb(const MatchJob &job) {
  const GridLayout &L = *job.L;
  const hipStream_t s = job.stream;
  NHIP_REQUIRE(bnb_fits(L, job.search), "csm_match: lattice %d x %d x %d beyond the branch-and-bound matcher's envelope",
               job.search->n_theta, job.search->nx, job.search->ny);
  if (job.n_pairs == 0) return NHIP_OK;
  const BnbPlan plan = bnb_plan(L, job.search, job.n_pairs, job.workspace ? job.workspace_bytes : 0);
  // (the general instantiation -- scans of more than 1088 points, NHIP_BNB_QUEUE=1 -- takes its exact sums on the row-major image)
  NHIP_REQUIRE(L.has_image || plan.short_scans, "csm_match: grids built with NHIP_GRID_NO_IMAGE serve lists whose scans all have at most %d "
               "points, and the caller must say so (NHIP_SEARCH_SHORT_SCANS; the handle API sets it itself)", NHIP_SHORT_SCAN_POINTS);
  BnbParams P;
  fill_bnb_params(P, job, plan);
  int rc = instr_buffers(plan, P, s);
  if (rc) return rc;
  if (plan.second) {  // (the hand-over lists in the workspace)
    P.rot_count = static_cast<uint32_t *>(job.workspace);
    P.rot_list = reinterpret_cast<RotEntry *>(static_cast<uint8_t *>(job.workspace) + BNB_WS_HEADER);
    NHIP_TRY_HIP(hipMemsetAsync(job.workspace, 0, BNB_WS_HEADER, s));
  }
  const BnbLaunchers K = plan.instrumented ? launchers_instr() : launchers_product();
  t_last_plan = plan;
  {
    TimerScope t_all(NHIP_TIMER_CSM, s);
    // (Tried and removed: the fused form's batch as K launches on K streams, so that one hardware queue's in-order
    //  dispatch does not keep free slots empty -- 2 / 4 / 8 queues took 10 / 30 / 45 % longer, profiles/r03_matcher_experiments.txt.)
    rc = plan.form == BNB_FUSED ? K.fused(P, plan, s) : run_rounds(P, plan, K, job.workspace, job.workspace_bytes, s);
  }
  if (rc) return rc;
  NHIP_TRY_HIP(hipGetLastError());
  launch_csm_finalize(job);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

// NHIP_BNB_STATS=1: (blocks evaluated exactly, blocks in all) since the last call; resets the counters
int bnb_stats_per_pair(unsigned long long *out, int32_t n) {
  if (!g_bnb_stats || n <= 0) return NHIP_OK;
  NHIP_TRY_HIP(hipMemcpy(out, g_bnb_stats + BNB_STATS_HEAD, 8 * (size_t)(n < BNB_STATS_PAIRS ? n : BNB_STATS_PAIRS), hipMemcpyDeviceToHost));
  return NHIP_OK;
}

int bnb_timeline_read(unsigned long long *out, int32_t n) {
  if (!g_bnb_timeline || n <= 0) return NHIP_OK;
  if (n > BNB_STATS_PAIRS) n = BNB_STATS_PAIRS;
  NHIP_TRY_HIP(hipMemcpy(out, g_bnb_timeline, 32 * (size_t)n, hipMemcpyDeviceToHost));
  // (the last pair's slot is followed by the second kernel's first start / last end)
  NHIP_TRY_HIP(hipMemcpy(out + 4 * (size_t)n, g_bnb_timeline + 4 * (size_t)BNB_STATS_PAIRS, 16, hipMemcpyDeviceToHost));
  return NHIP_OK;
}

int bnb_timeline_cand_read(unsigned long long *out, int32_t n) {  // out[0..n): first start, out[n..2n): last end
  if (!g_bnb_timeline || n <= 0) return NHIP_OK;
  if (n > BNB_STATS_PAIRS) n = BNB_STATS_PAIRS;
  NHIP_TRY_HIP(hipMemcpy(out, g_bnb_timeline + 4 * (size_t)BNB_STATS_PAIRS + 2, 8 * (size_t)n, hipMemcpyDeviceToHost));
  NHIP_TRY_HIP(hipMemcpy(out + n, g_bnb_timeline + 5 * (size_t)BNB_STATS_PAIRS + 2, 8 * (size_t)n, hipMemcpyDeviceToHost));
  return NHIP_OK;
}

int bnb_stats_read(unsigned long long out[24]) {
  static_assert(BNB_STATS_HEAD == 24, "the head is what nhip_bnb_stats_levels hands out");
  for (int i = 0; i < BNB_STATS_HEAD; i++) out[i] = 0;
  if (!g_bnb_stats) return NHIP_OK;
  NHIP_TRY_HIP(hipMemcpy(out, g_bnb_stats, 8 * BNB_STATS_HEAD, hipMemcpyDeviceToHost));
  NHIP_TRY_HIP(hipMemset(g_bnb_stats, 0, 8 * BNB_STATS_HEAD));
  return NHIP_OK;
}

int bnb_stats_chunks_read(unsigned long long out[4]) {
  for (int i = 0; i < BNB_STATS_CHUNKS; i++) out[i] = 0;
  if (!g_bnb_stats) return NHIP_OK;
  unsigned long long *at = g_bnb_stats + BNB_STATS_HEAD + (size_t)BNB_STATS_PAIRS;
  NHIP_TRY_HIP(hipMemcpy(out, at, 8 * BNB_STATS_CHUNKS, hipMemcpyDeviceToHost));
  NHIP_TRY_HIP(hipMemset(at, 0, 8 * BNB_STATS_CHUNKS));
  return NHIP_OK;
}

int bnb_stats_seeds_read(unsigned long long out[8]) {
  for (int i = 0; i < BNB_STATS_SEEDS; i++) out[i] = 0;
  if (!g_bnb_stats) return NHIP_OK;
  unsigned long long *at = g_bnb_stats + BNB_STATS_HEAD + (size_t)BNB_STATS_PAIRS + BNB_STATS_CHUNKS;
  NHIP_TRY_HIP(hipMemcpy(out, at, 8 * BNB_STATS_SEEDS, hipMemcpyDeviceToHost));
  NHIP_TRY_HIP(hipMemset(at, 0, 8 * BNB_STATS_SEEDS));
  return NHIP_OK;
}

}  // namespace nhip
