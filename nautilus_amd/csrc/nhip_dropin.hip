// nhip_dropin.hip -- the reference-shaped single-pair call, nhip_csm_get_transformation: the cache of the last targets'
// tables, the calling thread's scratch, one level after the other or both chained on the device (dropin_bridge_kernel).
#include <algorithm>
#include <cstddef>
#include <memory>

#include "nhip_common.h"
#include "nhip_csm_shared.h"  // (decode_key)
#include "nhip_host.h"

using namespace nhip;

// ---- the reference-shaped single-pair call, with the tables of the last targets kept
// Solver::SolveAutoLC -> GetRelativeTransform (solver.cc:630-649, 676-700) calls GetTransformation once per candidate pair,
// and a target scan is matched against many sources in a row.  A call used to zero and build 77 MB + 161 MB of tables
// for a target it had seen a call ago (1.4 ms, 708 calls/s); now the two grid handles of the last targets stay, keyed by
// the target cloud ITSELF (length + 64-bit hash to find it, the bytes compared to be sure) and the constructor's
// parameters, least recently used out first under a byte cap (nhip_csm_cache_configure / nhip_csm_cache_clear).
// The fine grid of a cached target is built for the largest reach any coarse optimum can ask for (its layout no longer
// depends on the source), which changes no result: the border is zeros either way.
namespace {

struct CachedTarget {
  std::vector<float> cloud;   // the target's points, for the exact comparison
  uint64_t hash = 0;
  nhip_csm_params_t params;
  int device = -1;
  nhip_grids_t *g1 = nullptr, *g2 = nullptr;
  nhip_grid_spec_t spec1, spec2;
  int64_t bytes = 0;
  ~CachedTarget() {
    if (g1) nhip_grids_free(g1);
    if (g2) nhip_grids_free(g2);
  }
};

std::mutex g_cache_mu;
// most recently used first.  (Heap-allocated and never destroyed: at process exit the HIP runtime may be gone before
// static destructors run, and freeing device memory then is not safe; nhip_csm_cache_clear() frees it while it is.)
std::vector<std::shared_ptr<CachedTarget>> &g_cache = *new std::vector<std::shared_ptr<CachedTarget>>();
int64_t g_cache_cap = 3ll << 30;
int64_t g_cache_hits = 0, g_cache_misses = 0;

uint64_t hash_bytes(const void *p, size_t n) {  // FNV-1a over 8-byte words (+ tail): finds the entry, never decides equality
  const uint8_t *b = static_cast<const uint8_t *>(p);
  uint64_t h = 1469598103934665603ull;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, b + i, 8);
    h = (h ^ w) * 1099511628211ull;
  }
  for (; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

bool same_params(const nhip_csm_params_t &a, const nhip_csm_params_t &b) {
  return a.scanner_range == b.scanner_range && a.trans_range == b.trans_range && a.low_res == b.low_res &&
         a.high_res == b.high_res && a.sigma == b.sigma && a.floor_p == b.floor_p &&
         (a.cell_bits == 0 ? 16 : a.cell_bits) == (b.cell_bits == 0 ? 16 : b.cell_bits);
}

// the entry of this target cloud (n points, hash h) under these parameters on this device
bool same_target(const CachedTarget &c, uint64_t h, int device, const nhip_csm_params_t &p, const float *cloud, int32_t n) {
  return c.hash == h && c.device == device && c.cloud.size() == 2 * (size_t)n && same_params(c.params, p) &&
         memcmp(c.cloud.data(), cloud, sizeof(float) * 2 * (size_t)n) == 0;
}

// the least recently used entries beyond the cap move to `drop` (under g_cache_mu; the caller frees them outside the lock)
void trim_cache(std::vector<std::shared_ptr<CachedTarget>> &drop) {
  int64_t tot = 0;
  size_t keep = 0;
  for (; keep < g_cache.size() && tot + g_cache[keep]->bytes <= g_cache_cap; keep++) tot += g_cache[keep]->bytes;
  drop.assign(g_cache.begin() + (long)keep, g_cache.end());
  g_cache.resize(keep);
}

// The calling thread's scratch for one pair (device buffers that live as long as the thread's library use: a call is
// two launches and four small copies, no allocation).
constexpr int DROPIN_PARTS_MAX = 8;  // "pairs" (workgroups) one search's rotations may be dealt over
struct DropInScratch {
  int device = -1;
  // par: one block of per-call parameters, uploaded in ONE copy {scan offsets int32[2] @0, (cos, sin) theta0 per part
  // double[16] @16, search centre per part int32[16] @144, rotation base per part int32[8] @208}; res: the records
  // nhip_match_t[8] @0 and their sums int32[8] @128, downloaded in one copy
  DevBuf xy, par, idx, keys, res, delta1, delta2, ws;
  // the chained form (both levels enqueued behind one another, ONE synchronisation per call): the fine level's parameter
  // block is written on the device by dropin_bridge_kernel from the coarse record and a table of the (cos, sin) every
  // coarse rotation would hand to the fine level (libm values, computed by the host per call); its keys, workspace and
  // records are its own, the host's blocks travel through pinned memory
  DevBuf par2, rot1, keys2, ws2;
  void *pin = nullptr;  // pinned host staging: upload block (256 B of parameters + the table) | download block (512 B)
  size_t xy_cap = 0;
  int32_t n_theta1 = -1, n_theta2 = -1;
  double step1 = 0, step2 = 0;
};
// (a few KB of device memory per calling thread, freed when the thread ends: thread-local destructors -- the main thread's
//  too -- run before the process's static destructors, i.e. while the HIP runtime is still there)
static thread_local double t_dropin_info[4] = {0, 0, 0, 0};
constexpr int DROPIN_CHAIN_ROT_MAX = 512;               // coarse rotations the chained form's table holds
// the upload block: the coarse level's DropInPar, at DROPIN_UP_TABLE the table; the download block (and DropInScratch::res
// behind it): the coarse level's DropInRes, the fine level's, the centre the fine search ran at (int32[2])
constexpr size_t DROPIN_PAR_BYTES = 256, DROPIN_UP_TABLE = DROPIN_PAR_BYTES;
constexpr size_t DROPIN_UP_BYTES = DROPIN_UP_TABLE + 16 * (size_t)DROPIN_CHAIN_ROT_MAX, DROPIN_DOWN_BYTES = 512;
constexpr size_t DROPIN_DOWN_RES2 = 256, DROPIN_DOWN_ORIGIN = 480;
struct ScratchHolder {
  DropInScratch *p = nullptr;
  ~ScratchHolder() {
    if (p && p->pin) (void)hipHostFree(p->pin);
    delete p;
  }
};
thread_local ScratchHolder t_scratch;

int scratch_for(int device, int32_t n_a, const nhip_search_t &s1, const nhip_search_t &s2, DropInScratch **out) {
  if (!t_scratch.p) t_scratch.p = new DropInScratch();
  DropInScratch &S = *t_scratch.p;
  int rc;
  // (a failure below leaves the scratch EMPTY -- device -1 -- so that the thread's next call sets it up again instead of
  //  finding the device it asked for and null buffers behind it)
  auto reset = [&S]() {
    if (S.pin) (void)hipHostFree(S.pin);
    S.~DropInScratch();
    new (&S) DropInScratch();
  };
  if (S.device != device) {
    reset();
    const int32_t zeros[2 * DROPIN_PARTS_MAX] = {0};
    constexpr size_t G = DROPIN_PARTS_MAX;
    if ((rc = S.par.alloc(DROPIN_PAR_BYTES)) || (rc = S.idx.alloc(8 * G)) || (rc = S.keys.alloc(8 * G)) || (rc = S.res.alloc(DROPIN_DOWN_BYTES)) ||
        (rc = S.ws.alloc((size_t)bnb_workspace_bytes_lists((int32_t)G))) || (rc = S.par2.alloc(DROPIN_PAR_BYTES)) ||
        (rc = S.rot1.alloc(DROPIN_UP_BYTES)) || (rc = S.keys2.alloc(8 * G)) ||
        (rc = S.ws2.alloc((size_t)bnb_workspace_bytes_lists((int32_t)G)))) {
      reset();
      return rc;
    }
    if (hipHostMalloc(&S.pin, DROPIN_UP_BYTES + DROPIN_DOWN_BYTES, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      S.pin = nullptr;  // (no pinned memory: the call falls back to the form with one synchronisation per level)
    }
    const hipError_t e = hipMemcpy(S.idx.p, zeros, 8 * G, hipMemcpyHostToDevice);  // source scan 0, grid slot 0 for every part
    if (e != hipSuccess) {
      reset();
      return hip_fail(e, "csm_get_transformation scratch", __FILE__, __LINE__);
    }
    S.device = device;
  }
  if ((size_t)n_a > S.xy_cap) {
    const size_t cap = std::max<size_t>((size_t)n_a, 2048);
    S.xy_cap = 0;  // (DevBuf::alloc frees first: a failed allocation leaves no buffer, and no capacity that says otherwise)
    if ((rc = S.xy.alloc(sizeof(float) * 2 * cap))) return rc;
    S.xy_cap = cap;
  }
  auto table = [&](DevBuf &d, int32_t &n_have, double &step_have, const nhip_search_t &s) -> int {
    if (n_have == s.n_theta && step_have == s.theta_step) return NHIP_OK;
    // (+ DROPIN_PARTS_MAX copies of the last rotation: a search dealt over several workgroups in equal parts reads past
    //  the table's end; a copy's poses tie with the original's and lose the tie by their larger index)
    std::vector<double> t(2 * (size_t)(s.n_theta + DROPIN_PARTS_MAX));
    int r = nhip_csm_delta_table(&s, t.data());
    if (r) return r;
    for (int e = 0; e < DROPIN_PARTS_MAX; e++) {
      t[2 * (size_t)(s.n_theta + e)] = t[2 * (size_t)(s.n_theta - 1)];
      t[2 * (size_t)(s.n_theta + e) + 1] = t[2 * (size_t)(s.n_theta - 1) + 1];
    }
    if ((r = d.alloc(sizeof(double) * t.size()))) return r;
    NHIP_TRY_HIP(hipMemcpy(d.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
    n_have = s.n_theta;
    step_have = s.theta_step;
    return NHIP_OK;
  };
  if ((rc = table(S.delta1, S.n_theta1, S.step1, s1)) || (rc = table(S.delta2, S.n_theta2, S.step2, s2))) return rc;
  *out = &S;
  return NHIP_OK;
}

// The per-call blocks of one level: scan 0 of the scratch against slot 0 of its grids, on the null stream.
struct DropInPar {  // the per-call parameter block as the kernels read it (device copy: DropInScratch::par / par2)
  int32_t off[4];   // scan offsets {0, n_a}
  double cs[2 * DROPIN_PARTS_MAX];   // (cos, sin) theta0 per part
  int32_t org[2 * DROPIN_PARTS_MAX], kb[DROPIN_PARTS_MAX];  // search centre per part, rotation base per part
};
static_assert(sizeof(DropInPar) == 240 && offsetof(DropInPar, off) == 0 && offsetof(DropInPar, cs) == 16 && offsetof(DropInPar, org) == 144 &&
              offsetof(DropInPar, kb) == 208 && sizeof(DropInPar) <= DROPIN_PAR_BYTES, "DropInPar layout");
struct DropInRes {
  nhip_match_t rec[DROPIN_PARTS_MAX];
  int32_t sums[DROPIN_PARTS_MAX];
};
static_assert(sizeof(DropInRes) == 160 && offsetof(DropInRes, sums) == 128, "DropInRes layout");
static_assert(sizeof(DropInRes) <= DROPIN_DOWN_RES2 && DROPIN_DOWN_RES2 + sizeof(DropInRes) <= DROPIN_DOWN_ORIGIN &&
              DROPIN_DOWN_ORIGIN + 2 * sizeof(int32_t) <= DROPIN_DOWN_BYTES, "download block layout");

// One level of a call: its search on grids `g` and the plan for it.  The branch-and-bound matcher computes a pair's bounds
// in the pair's ONE workgroup, eight rotations at a time: a search of 21 rotations is three rounds on one CU while 255 idle.
// So its rotations are dealt over `parts` workgroups of `per` -- the fewest parts (2 .. 8) that give every workgroup an odd
// number (the lattice's rule) of at most 8.  To the kernels they are `parts` pairs of the same scan and table whose rotation
// 0 is entry kbase of the rotation table (BnbParams::pair_kbase), and the host takes the best of their records: the larger
// sum, on a tie the smaller index ((k * nx + ix) * ny + iy with the part's rotations counted from the search's first), which
// is the one-workgroup result.  Every other form takes the search as one pair.
struct DropInLevel {
  nhip_grids_t *g = nullptr;
  nhip_search_t s = {};
  MatchPlan plan;
  int parts = 1, per = 0;
  DropInLevel() = default;
  DropInLevel(nhip_grids_t *g_, const nhip_search_t &s_) : g(g_), s(s_), plan(csm_plan(g_->L, &s_, 1)), per(s_.n_theta) {
    if (plan.form == MATCH_BNB && s.n_theta > 8)
      for (int q = 2; q <= DROPIN_PARTS_MAX; q++) {
        const int r = (s.n_theta + q - 1) / q;
        if ((r & 1) && r <= 8) {
          parts = q;
          per = r;
          break;
        }
      }
  }
};

// enqueue one level: parameters in the device block `d_par` (DropInPar), records into the device block `d_res` (DropInRes)
int dropin_enqueue(DropInScratch &S, int32_t n_a, const DropInLevel &v, const nhip_grid_spec_t &spec_now, const DevBuf &d_delta,
                   const DevBuf &d_par, bool with_origin, const DevBuf &d_keys, const DevBuf &d_ws, uint8_t *dr) {
  const uint8_t *dp = d_par.as<const uint8_t>();
  nhip_search_t part = v.s;
  part.n_theta = v.per;
  // (the host holds the cloud: a source that fits the matcher's by-rotation form saves the launch of the other instantiation)
  if (n_a <= NHIP_SHORT_SCAN_POINTS) part.flags |= NHIP_SEARCH_SHORT_SCANS;
  MatchJob job = job_on(S.xy, d_par, *v.g, spec_now);  // (the scan offsets are the block's first member, DropInPar::off)
  job.ids = {1, v.g->n, dev_status()};  // (the scratch holds one scan; every part reads scan 0, slot 0)
  job.pair_src = S.idx.as<const int32_t>();
  job.pair_slot = S.idx.as<const int32_t>() + DROPIN_PARTS_MAX;
  job.rot0_cs = reinterpret_cast<const double *>(dp + offsetof(DropInPar, cs));
  job.delta_cs = d_delta.as<const double>();
  if (with_origin) job.pair_origin = reinterpret_cast<const int32_t *>(dp + offsetof(DropInPar, org));
  if (v.parts > 1) job.pair_kbase = reinterpret_cast<const int32_t *>(dp + offsetof(DropInPar, kb));
  job.n_pairs = v.parts;
  job.search = &part;
  job.keys = d_keys.as<uint64_t>();
  job.out = reinterpret_cast<nhip_match_t *>(dr + offsetof(DropInRes, rec));
  job.sums = reinterpret_cast<int32_t *>(dr + offsetof(DropInRes, sums));
  job.workspace = d_ws.p;
  job.workspace_bytes = (int64_t)d_ws.bytes;
  return launch_csm_match(job, v.plan);
}

// the best of the parts' records
void dropin_pick(DropInRes &res, const DropInLevel &v, nhip_match_t *m) {
  int best = -1;
  int64_t best_lin = 0;
  for (int q = 0; q < v.parts; q++) {
    // (a copy of the last rotation past the table's end IS the last rotation)
    res.rec[q].itheta = std::min(res.rec[q].itheta + q * v.per, v.s.n_theta - 1);
    const int64_t lin = ((int64_t)res.rec[q].itheta * v.s.nx + res.rec[q].ix) * v.s.ny + res.rec[q].iy;
    if (best < 0 || res.sums[q] > res.sums[best] || (res.sums[q] == res.sums[best] && lin < best_lin)) {
      best = q;
      best_lin = lin;
    }
  }
  *m = res.rec[best];
}

// One level with the host after it: the record comes back to the host.
int match_one(DropInScratch &S, int32_t n_a, const DropInLevel &v, const DevBuf &d_delta, double theta0, const int32_t *origin,
              nhip_match_t *m) {
  int rc = ensure_skip_maps(v.g, v.plan);
  if (rc) return rc;
  nhip_grid_spec_t spec_now;
  spec_under_lock(v.g, &spec_now);
  DropInPar par;
  memset(&par, 0, sizeof(par));
  par.off[1] = n_a;
  if ((rc = nhip_csm_rot0(&theta0, nullptr, 1, par.cs))) return rc;
  for (int q = 0; q < v.parts; q++) {
    par.cs[2 * q] = par.cs[0];
    par.cs[2 * q + 1] = par.cs[1];
    par.org[2 * q] = origin ? origin[0] : 0;
    par.org[2 * q + 1] = origin ? origin[1] : 0;
    par.kb[q] = q * v.per;
  }
  NHIP_TRY_HIP(hipMemcpyAsync(S.par.p, &par, sizeof(par), hipMemcpyHostToDevice, nullptr));
  if ((rc = dropin_enqueue(S, n_a, v, spec_now, d_delta, S.par, origin != nullptr, S.keys, S.ws, S.res.as<uint8_t>()))) return rc;
  DropInRes res;
  NHIP_TRY_HIP(hipMemcpy(&res, S.res.p, sizeof(res), hipMemcpyDeviceToHost));
  dropin_pick(res, v, m);
  return NHIP_OK;
}

// The fine level's parameter block from the coarse level's record, on the device (one thread): the same arithmetic as
// nhip_match_to_transform + the host code between the two levels -- products and quotients of doubles, individually
// rounded (the library is compiled with -ffp-contract=off), conversions to float by round-to-nearest, lround -- so the host,
// which repeats it on the downloaded coarse record to report the transform, arrives at the same origin.  The (cos, sin) of
// the fine search's centre angle are NOT computed here: device and host libm differ in the last place; the host tabulates
// its own values for every coarse rotation and the kernel picks the winner's.
extern "C" __global__ void dropin_bridge_kernel(const nhip_match_t *rec1, const double *rot1, int32_t hx1, int32_t hy1, double low_res,
                                     double high_res, int32_t n_a, int32_t parts2, int32_t per2, DropInPar *par2, int32_t *info,
                                     const unsigned long long *keys1, int32_t nx1, int32_t ny1, double Lf1, double step1,
                                     nhip_match_t *rec1_out, int32_t *sums1_out, unsigned long long *keys2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  nhip_match_t m;
  if (keys1) {
    // the coarse search left its keys undecoded (MatchPlan::keys_undecoded): csm_finalize_kernel's decoding, here, and the
    // fine search's keys zeroed for it (keys_zeroed) -- two small launches and a memset fewer per call
    const unsigned long long key = keys1[0];
    const uint32_t sum = (uint32_t)(key >> 32);
    decode_key(key, nx1, ny1, m);
    double sc = Lf1;
    if (n_a > 0) sc = __dadd_rn(Lf1, __ddiv_rn(__dmul_rn(step1, (double)sum), (double)n_a));
    m.score = __double2float_rn(sc);
    rec1_out[0] = m;
    sums1_out[0] = (int32_t)sum;
    for (int q = 0; q < DROPIN_PARTS_MAX; q++) keys2[q] = 0ull;
  } else {
    m = rec1[0];
  }
  const float tx1 = __double2float_rn(__dmul_rn((double)(m.ix - hx1), low_res));
  const float ty1 = __double2float_rn(__dmul_rn((double)(m.iy - hy1), low_res));
  const int32_t ox = (int32_t)lround(__ddiv_rn((double)tx1, high_res)), oy = (int32_t)lround(__ddiv_rn((double)ty1, high_res));
  par2->off[0] = 0;
  par2->off[1] = n_a;
  par2->off[2] = par2->off[3] = 0;
  const int32_t k = m.itheta < 0 ? 0 : (m.itheta >= DROPIN_CHAIN_ROT_MAX ? DROPIN_CHAIN_ROT_MAX - 1 : m.itheta);
  const double c = rot1[2 * k], s_ = rot1[2 * k + 1];
  for (int q = 0; q < DROPIN_PARTS_MAX; q++) {
    par2->cs[2 * q] = c;
    par2->cs[2 * q + 1] = s_;
    par2->org[2 * q] = ox;
    par2->org[2 * q + 1] = oy;
    par2->kb[q] = q < parts2 ? q * per2 : 0;
  }
  info[0] = ox;
  info[1] = oy;
}

// Both levels behind one another on the null stream, ONE synchronisation: upload (source cloud; coarse parameters + the
// table of fine-centre rotations, one pinned block), coarse search, bridge, fine search (+ exact score), download of both
// levels' records and of the centre the fine search ran at in one pinned block.  Same records as two match_one calls
// (tests/test_csm_gpu.py, test_adapters_gpu.py compare the call with the oracle's two-level search float for float).  The
// caller has checked that the form applies: pinned staging, a coarse search in one part of at most DROPIN_CHAIN_ROT_MAX
// rotations.
int match_chained(DropInScratch &S, const float *pc_a, int32_t n_a, const DropInLevel &c1, const DropInLevel &c2, double low_res,
                  double high_res, double theta0, nhip_match_t *m1, nhip_match_t *m2, int32_t dev_origin[2]) {
  int rc;
  if ((rc = ensure_skip_maps(c1.g, c1.plan)) || (rc = ensure_skip_maps(c2.g, c2.plan))) return rc;
  nhip_grid_spec_t spec1_now, spec2_now;
  spec_under_lock(c1.g, &spec1_now);
  spec_under_lock(c2.g, &spec2_now);
  const nhip_search_t &s1 = c1.s;
  uint8_t *up = static_cast<uint8_t *>(S.pin), *down = up + DROPIN_UP_BYTES;
  DropInPar *par1 = reinterpret_cast<DropInPar *>(up);
  memset(par1, 0, sizeof(*par1));
  par1->off[1] = n_a;
  if ((rc = nhip_csm_rot0(&theta0, nullptr, 1, par1->cs))) return rc;
  // what the host would hand the fine level for each coarse rotation k: theta1 = (double)(float)(theta0 + (k - half) * step)
  double *rot = reinterpret_cast<double *>(up + DROPIN_UP_TABLE);
  const int32_t half1 = (s1.n_theta - 1) / 2;
  for (int32_t k = 0; k < s1.n_theta; k++) {
    const double theta1 = (double)(float)(theta0 + (double)(k - half1) * s1.theta_step);
    if ((rc = nhip_csm_rot0(&theta1, nullptr, 1, rot + 2 * k))) return rc;
  }
  const size_t up_bytes = DROPIN_UP_TABLE + 16 * (size_t)s1.n_theta;
  if (n_a) NHIP_TRY_HIP(hipMemcpyAsync(S.xy.p, pc_a, sizeof(float) * 2 * (size_t)n_a, hipMemcpyHostToDevice, nullptr));
  NHIP_TRY_HIP(hipMemcpyAsync(S.rot1.p, up, up_bytes, hipMemcpyHostToDevice, nullptr));
  uint8_t *dres = S.res.as<uint8_t>();
  // both levels through the kernel whose lanes are poses (the default): the bridge decodes the coarse keys and zeroes the fine
  // ones, the exact-score pass decodes the fine keys -- no finalize launches, no second memset
  const bool fused = c1.plan.form == MATCH_POSES && c2.plan.form == MATCH_POSES && (c2.s.flags & NHIP_SEARCH_EXACT_SCORE);
  DropInLevel v1 = c1, v2 = c2;
  v1.plan.keys_undecoded = v2.plan.keys_zeroed = v2.plan.keys_undecoded = fused;
  if ((rc = dropin_enqueue(S, n_a, v1, spec1_now, S.delta1, S.rot1, false, S.keys, S.ws, dres))) return rc;
  hipLaunchKernelGGL(dropin_bridge_kernel, dim3(1), dim3(64), 0, nullptr, reinterpret_cast<const nhip_match_t *>(dres),
                     reinterpret_cast<const double *>(S.rot1.as<uint8_t>() + DROPIN_UP_TABLE), (s1.nx - 1) / 2, (s1.ny - 1) / 2,
                     low_res, high_res, n_a, c2.parts, c2.per, S.par2.as<DropInPar>(),
                     reinterpret_cast<int32_t *>(dres + DROPIN_DOWN_ORIGIN),
                     fused ? S.keys.as<const unsigned long long>() : nullptr, s1.nx, s1.ny, c1.g->L.Lf, c1.g->L.step,
                     reinterpret_cast<nhip_match_t *>(dres + offsetof(DropInRes, rec)),
                     reinterpret_cast<int32_t *>(dres + offsetof(DropInRes, sums)), S.keys2.as<unsigned long long>());
  NHIP_TRY_HIP(hipGetLastError());
  if ((rc = dropin_enqueue(S, n_a, v2, spec2_now, S.delta2, S.par2, true, S.keys2, S.ws2, dres + DROPIN_DOWN_RES2))) return rc;
  NHIP_TRY_HIP(hipMemcpyAsync(down, dres, DROPIN_DOWN_BYTES, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipStreamSynchronize(nullptr));
  DropInRes r1, r2;
  memcpy(&r1, down, sizeof(r1));
  memcpy(&r2, down + DROPIN_DOWN_RES2, sizeof(r2));
  memcpy(dev_origin, down + DROPIN_DOWN_ORIGIN, 2 * sizeof(int32_t));
  dropin_pick(r1, c1, m1);
  dropin_pick(r2, c2, m2);
  return NHIP_OK;
}

}  // namespace

extern "C" {

int nhip_csm_cache_configure(int64_t max_bytes) {
  NHIP_REQUIRE(max_bytes >= 0, "csm_cache_configure: negative size");
  std::vector<std::shared_ptr<CachedTarget>> drop;  // (freed outside the lock)
  std::lock_guard<std::mutex> lock(g_cache_mu);
  g_cache_cap = max_bytes;
  trim_cache(drop);
  return NHIP_OK;
}

int nhip_csm_cache_clear(void) {
  std::vector<std::shared_ptr<CachedTarget>> drop;
  std::lock_guard<std::mutex> lock(g_cache_mu);
  drop.swap(g_cache);
  return NHIP_OK;
}

int nhip_csm_cache_stats(int64_t *entries, int64_t *bytes, int64_t *hits, int64_t *misses) {
  std::lock_guard<std::mutex> lock(g_cache_mu);
  int64_t tot = 0;
  for (auto &e : g_cache) tot += e->bytes;
  if (entries) *entries = (int64_t)g_cache.size();
  if (bytes) *bytes = tot;
  if (hits) *hits = g_cache_hits;
  if (misses) *misses = g_cache_misses;
  return NHIP_OK;
}

int nhip_csm_get_transformation_info(double out[4]) {
  NHIP_REQUIRE(out != nullptr, "csm_get_transformation_info: null out");
  for (int i = 0; i < 4; i++) out[i] = t_dropin_info[i];
  return NHIP_OK;
}

int nhip_csm_get_transformation(const nhip_csm_params_t *p, const float *pc_a, int32_t n_a, const float *pc_b,
                                int32_t n_b, double rot_a, double rot_b, double rot_restriction, double *score,
                                float *tx, float *ty, float *theta) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(p && score && tx && ty && theta && n_a >= 0 && n_b >= 0 && (pc_a || n_a == 0) && (pc_b || n_b == 0),
               "csm_get_transformation: bad arguments");
  NHIP_REQUIRE(p->low_res > 0 && p->high_res > 0 && p->low_res >= p->high_res && p->trans_range >= 0 && rot_restriction >= 0,
               "csm_get_transformation: bad search parameters");
  const int32_t bits = p->cell_bits == 0 ? 16 : p->cell_bits;
  // (sums are int32, as in nhip_csm_match: the longest source cloud whose largest possible sum fits)
  NHIP_REQUIRE((int64_t)n_a <= 0x7fffffffll / (bits == 16 ? 65535 : 255), "csm_get_transformation: pc_a has %d points; with %d-bit "
               "cells at most %lld fit the int32 sums", n_a, bits, (long long)(0x7fffffffll / (bits == 16 ? 65535 : 255)));
  int device = 0;
  NHIP_TRY_HIP(hipGetDevice(&device));
  double theta0 = rot_a - rot_b;  // math_util.h:81-89 AngleDiff
  theta0 -= (2.0 * M_PI) * rint(theta0 / (2.0 * M_PI));
  const double coarse_step = M_PI / 180.0;
  // level 1: low_res grid, whole translation range, +-rot_restriction
  const int32_t h1 = (int32_t)floor(p->trans_range / p->low_res);
  const nhip_grid_spec_t spec1 = {p->scanner_range, p->low_res, p->sigma, p->floor_p, h1, bits, 0, 0};
  // (The coarse lattice is many rotations of few translations -- 181 x 13 x 13 at the reference's constants: the kernel that
  //  performs every add spreads its rotations over the whole chip, where the branch-and-bound matcher would compute the
  //  bounds of all of them in the pair's ONE workgroup, 23 rounds of its eight waves.  Same records either way.)
  const nhip_search_t s1 = {2 * (int32_t)floor(rot_restriction / coarse_step) + 1, 2 * h1 + 1, 2 * h1 + 1,
                            (2 * h1 + 1) <= 21 ? NHIP_SEARCH_EXHAUSTIVE : 0, coarse_step};
  // level 2: high_res grid, +-low_res around the coarse optimum, +-1 coarse step in 0.1 steps.  Its tables are built for
  // the largest search centre a coarse optimum can produce (+ the fine half-width), so that they serve every source.
  const int32_t ratio = (int32_t)lround(p->low_res / p->high_res);
  const int32_t reach_max = (int32_t)lround((double)h1 * p->low_res / p->high_res) + ratio + 2;
  // (the score the call returns is the fine optimum's on the UNQUANTISED table -- NHIP_SEARCH_EXACT_SCORE: the reference's
  //  table holds doubles, cimg_debug.h:19; both searches run on the quantised tables)
  // The fine level performs EVERY add, in the kernel whose lanes are poses (NHIP_SEARCH_LATENCY: 21 x 16 tiles of four rows of
  // the 61 x 61 plane, ~45 us whatever the clouds; where the tiles do not fit -- a low_res / high_res ratio of ~64 and more --
  // the strip kernels).  Round 6 measured the alternatives (profiles/r06_dropin_fine_level.txt): the branch-and-bound matcher
  // takes 110 us where the clouds match and 0.8-10 ms where they do not -- a flat landscape leaves it thousands of candidate
  // blocks on a table whose pooled level does not fit LDS; the strip kernels 0.16-0.48 ms.  Same records in every form.
  const nhip_search_t s2 = {21, 2 * ratio + 1, 2 * ratio + 1, NHIP_SEARCH_EXACT_SCORE | NHIP_SEARCH_EXHAUSTIVE | NHIP_SEARCH_LATENCY,
                            coarse_step / 10.0};
  // (a target whose fine tables would exceed the common reach, or an empty one, is not cached: its fine table is built for
  //  this call's coarse optimum alone, below)
  const bool cacheable = reach_max <= 4096 && n_b > 0;

  // ---- the target's tables: from the cache, or built now
  std::shared_ptr<CachedTarget> T;
  const uint64_t h = cacheable ? hash_bytes(pc_b, sizeof(float) * 2 * (size_t)n_b) ^ (uint64_t)n_b : 0;
  if (cacheable) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    for (size_t i = 0; i < g_cache.size(); i++)
      if (same_target(*g_cache[i], h, device, *p, pc_b, n_b)) {
        T = g_cache[i];
        g_cache.erase(g_cache.begin() + (long)i);
        g_cache.insert(g_cache.begin(), T);
        g_cache_hits++;
        break;
      }
    if (!T) g_cache_misses++;
  }
  const int32_t target = 0;
  std::unique_ptr<nhip_scans_t, int (*)(nhip_scans_t *)> bs(nullptr, nhip_scans_free);  // (the target's scans, while needed)
  if (!T) {
    T = std::make_shared<CachedTarget>();
    T->hash = h;
    T->params = *p;
    T->device = device;
    if (n_b) T->cloud.assign(pc_b, pc_b + 2 * (size_t)n_b);
    const int32_t off[2] = {0, n_b};
    nhip_scans_t *up = nullptr;
    if ((rc = nhip_scans_upload(pc_b, off, 1, &up))) return rc;
    bs.reset(up);
    T->spec1 = spec1;
    if ((rc = nhip_grids_build(bs.get(), &target, 1, &spec1, &T->g1))) return rc;
    if (cacheable) {
      T->spec2 = {p->scanner_range, p->high_res, p->sigma, p->floor_p, reach_max, bits, 0, 0};
      if ((rc = nhip_grids_build(bs.get(), &target, 1, &T->spec2, &T->g2))) return rc;
      bs.reset();
      T->bytes = (int64_t)T->g1->grids.bytes + (int64_t)T->g2->grids.bytes;
      std::vector<std::shared_ptr<CachedTarget>> drop;  // (evicted entries are freed outside the lock; a thread still matching
      {                                                  //  against one keeps it alive through its own shared_ptr)
        std::lock_guard<std::mutex> lock(g_cache_mu);
        // (two threads that missed on the same target at once both built it: the second finds the first's entry and keeps
        //  its own tables for this call only, so that no target counts twice against the cap)
        bool have = false;
        for (auto &c : g_cache) have = have || same_target(*c, h, device, *p, pc_b, n_b);
        if (!have && T->bytes <= g_cache_cap) {
          g_cache.insert(g_cache.begin(), T);
          trim_cache(drop);
        }
      }
    }
  }

  // ---- the two searches of this source.  Chained on the device where the form applies -- upload, coarse search, bridge
  // kernel (the fine level's parameter block from the coarse record), fine search, exact score, ONE download, ONE
  // synchronisation: the fine tables exist before the coarse search (a cached target), pinned staging, a coarse search in
  // one part of at most DROPIN_CHAIN_ROT_MAX rotations.  Otherwise one level after the other with the host in between.
  DropInScratch *S = nullptr;
  if ((rc = scratch_for(device, n_a, s1, s2, &S))) return rc;
  const DropInLevel c1(T->g1, s1);
  DropInLevel c2 = cacheable ? DropInLevel(T->g2, s2) : DropInLevel();
  const bool chained = cacheable && S->pin && s1.n_theta <= DROPIN_CHAIN_ROT_MAX && c1.parts == 1;
  nhip_match_t m1, m2;
  int32_t dev_origin[2] = {0, 0};
  if (chained) {
    if ((rc = match_chained(*S, pc_a, n_a, c1, c2, p->low_res, p->high_res, theta0, &m1, &m2, dev_origin))) return rc;
  } else {
    if (n_a) NHIP_TRY_HIP(hipMemcpyAsync(S->xy.p, pc_a, sizeof(float) * 2 * (size_t)n_a, hipMemcpyHostToDevice, nullptr));
    if ((rc = match_one(*S, n_a, c1, S->delta1, theta0, nullptr, &m1))) return rc;
  }
  float tx1, ty1, th1;
  if ((rc = nhip_match_to_transform(&m1, &spec1, &s1, theta0, 0, 0, &tx1, &ty1, &th1))) return rc;
  const int32_t origin[2] = {(int32_t)lround((double)tx1 / p->high_res), (int32_t)lround((double)ty1 / p->high_res)};
  if (!cacheable) {
    T->spec2 = {p->scanner_range, p->high_res, p->sigma, p->floor_p, std::max(abs(origin[0]), abs(origin[1])) + ratio, bits, 0, 0};
    if ((rc = nhip_grids_build(bs.get(), &target, 1, &T->spec2, &T->g2))) return rc;
    c2 = DropInLevel(T->g2, s2);
  }
  NHIP_REQUIRE(std::max(abs(origin[0]), abs(origin[1])) + ratio <= T->spec2.max_shift, "csm_get_transformation: coarse optimum "
               "(%d, %d) beyond the fine tables' reach %d", origin[0], origin[1], T->spec2.max_shift);
  // (the chained fine search ran at the centre dropin_bridge_kernel derived on the device from the same record: the
  //  transform below is built around the host's, so the two must agree)
  NHIP_REQUIRE(!chained || (dev_origin[0] == origin[0] && dev_origin[1] == origin[1]), "csm_get_transformation: the fine search "
               "ran around (%d, %d) on the device, the coarse optimum is at (%d, %d) on the host", dev_origin[0], dev_origin[1],
               origin[0], origin[1]);
  const double theta1 = th1;
  if (!chained && (rc = match_one(*S, n_a, c2, S->delta2, theta1, origin, &m2))) return rc;
  t_dropin_info[0] = (double)m1.score;
  t_dropin_info[1] = c2.plan.form == MATCH_BNB ? 0.0 : (c2.plan.form == MATCH_POSES ? 2.0 : 1.0);
  t_dropin_info[2] = chained ? 1.0 : 0.0;
  t_dropin_info[3] = (double)m1.itheta;
  if ((rc = nhip_match_to_transform(&m2, &T->spec2, &s2, theta1, origin[0], origin[1], tx, ty, theta))) return rc;
  *score = (double)m2.score;
  return NHIP_OK;
}

}  // extern "C"
