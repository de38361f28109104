// nhip_csm_plan.hip -- host side of the scan matcher's searches: which kernel takes a search (csm_plan), what every search
// must satisfy (check_search), the dispatch on the plan (launch_csm_match) and the launchers of the strip kernels, whose
// device side is nhip_csm_strip.h with a unit per cell width (nhip_csm.hip, nhip_csm16.hip).
#include "nhip_csm_shared.h"

namespace nhip {

namespace {

using namespace csm;

int check_search(const nhip_grid_spec_t *spec, const GridLayout &L, const nhip_search_t *search) {
  NHIP_REQUIRE(search->n_theta >= 1 && (search->n_theta & 1), "search: n_theta must be odd >= 1");
  NHIP_REQUIRE(search->nx >= 1 && (search->nx & 1), "search: nx must be odd >= 1");
  NHIP_REQUIRE(search->ny >= 1 && (search->ny & 1), "search: ny must be odd >= 1");
  NHIP_REQUIRE((search->nx - 1) / 2 <= spec->max_shift && (search->ny - 1) / 2 <= spec->max_shift,
               "search: shifts +-%d/+-%d exceed the grids' max_shift %d", (search->nx - 1) / 2,
               (search->ny - 1) / 2, spec->max_shift);
  NHIP_REQUIRE((int64_t)search->n_theta * search->nx * search->ny < 0x7fffffffll,
               "search: lattice too large for 32-bit linear index");
  NHIP_REQUIRE(L.S + 2 * L.pad < 65536, "search: stored grid side %d does not fit 16-bit cell packing",
               L.S + 2 * L.pad);
  NHIP_REQUIRE(L.pitch % 16 == 0, "search: grid pitch must be a multiple of 16");
  return NHIP_OK;
}

// the strip kernels' parameters: the job's, the blocks of the plane and the dense rule
void fill_params(CsmParams &P, const MatchJob &job, const StripKernels &K) {
  fill_job_params(P, job);
  P.npbx = (P.nx + K.pb_nx - 1) / K.pb_nx;
  P.npby = (P.ny + K.pb_ny - 1) / K.pb_ny;
  // NHIP_CSM_DENSE=1 switches the zero-strip skipping off (measurement: the same kernel, every add done), and so does the
  // search's flag.  16-bit grids are built without a skip map unless the spec asks (the matcher's product path never reads
  // it): without one every strip is added.  8-bit grids always carry theirs.
  const char *dense = tunable("NHIP_CSM_DENSE");
  const bool no_map = job.L->cb == 2 && !(job.spec->flags & NHIP_GRID_SKIP_MAP);
  P.dense = ((dense && dense[0] == '1') || (job.search->flags & NHIP_SEARCH_DENSE) || no_map) ? 1 : 0;
}

const StripKernels &strip_kernels(const GridLayout &L) { return L.cb == 2 ? strip_kernels16() : strip_kernels8(); }

int launch_strip_match(const MatchJob &job) {
  const StripKernels &K = strip_kernels(*job.L);
  const hipStream_t s = job.stream;
  CsmParams P;
  fill_params(P, job, K);
  P.keys = reinterpret_cast<unsigned long long *>(job.keys);
  const int64_t per_pair = (int64_t)P.n_theta * P.npbx * P.npby;
  const int64_t blocks = ((int64_t)(job.n_pairs + 7) / 8) * 8 * per_pair;
  NHIP_REQUIRE(blocks < 0x7fffffffll, "csm_match: %lld workgroups exceed one launch; split the batch",
               (long long)blocks);
  NHIP_TRY_HIP(hipMemsetAsync(job.keys, 0, sizeof(uint64_t) * (size_t)job.n_pairs, s));
  timer_begin(NHIP_TIMER_CSM, s);
  hipLaunchKernelGGL(K.match[P.dense], dim3((uint32_t)blocks), dim3(K.threads), 0, s, P);
  timer_end(NHIP_TIMER_CSM, s);
  launch_csm_finalize(job);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace

MatchPlan csm_plan(const GridLayout &L, const nhip_search_t *search, int32_t n_pairs) {
  MatchPlan plan;
  // branch and bound unless every add is asked for (NHIP_CSM_EXHAUSTIVE=1: tests) or the lattice is beyond its envelope
  const char *ex = tunable("NHIP_CSM_EXHAUSTIVE");
  if (!(search->flags & NHIP_SEARCH_EXHAUSTIVE) && !(ex && ex[0] == '1') && bnb_fits(L, search)) return plan;
  // every add: planes of few translations (the coarse level of GetTransformation: 13 x 13) in the kernel whose lanes are
  // poses; so, for lists of a few pairs (NHIP_SEARCH_LATENCY), larger planes in tiles of whole rows (the fine level).
  // NHIP_CSM_SMALL=0 (tests): the strip kernels for these lattices too.
  const char *sm = tunable("NHIP_CSM_SMALL");
  if (!(sm && sm[0] == '0')) {
    plan.form = MATCH_POSES;
    if (csm_small_plane_fits(search)) {
      plan.tile_rows = search->ny;
      plan.n_tiles = 1;
      return plan;
    }
    if ((search->flags & NHIP_SEARCH_LATENCY) && csm_small_tiled_fits(search, n_pairs, &plan.tile_rows, &plan.n_tiles)) return plan;
  }
  plan.form = L.cb == 2 ? MATCH_STRIPS16 : MATCH_STRIPS8;
  plan.tile_rows = plan.n_tiles = 0;
  return plan;
}


int launch_csm_match(const MatchJob &job, const MatchPlan &plan) {
  const GridLayout &L = *job.L;
  // (per-pair offsets into the rotation table are the branch-and-bound matcher's: an internal caller that passes them has
  //  made sure the lattice is one it takes)
  NHIP_REQUIRE(!job.pair_kbase || plan.form == MATCH_BNB, "csm_match: rotation offsets per pair with a lattice the matcher does not take");
  int rc = check_search(job.spec, L, job.search);
  if (rc) return rc;
  // (what the exact-score pass requires of the grids, before the search it follows is launched: a refused call writes nothing)
  NHIP_REQUIRE(!(job.search->flags & NHIP_SEARCH_EXACT_SCORE) || L.R <= 15, "csm_match: NHIP_SEARCH_EXACT_SCORE reads row "
               "windows of at most 31 bits; the grids' blur radius %d > 15 (sigma > 5 cells)", L.R);
  NHIP_REQUIRE(L.has_image || plan.form == MATCH_BNB, "csm_match: this search takes the kernel that performs every add "
               "(NHIP_SEARCH_EXHAUSTIVE, or a lattice beyond the branch-and-bound matcher's envelope), which reads the row-major "
               "image the grids were built without (NHIP_GRID_NO_IMAGE)");
  if (job.n_pairs == 0) return NHIP_OK;
  switch (plan.form) {
    case MATCH_BNB: rc = launch_csm_bnb(job); break;  // the same records, most adds never performed (nhip_bnb.hip)
    case MATCH_POSES: rc = launch_csm_small_match(job, plan); break;
    case MATCH_STRIPS16:
    case MATCH_STRIPS8: rc = launch_strip_match(job); break;  // (the plan's form follows the grids' cell width)
  }
  if (rc || !(job.search->flags & NHIP_SEARCH_EXACT_SCORE)) return rc;
  // (the records are final -- indices and integer sums; the pass replaces their score field.  A search that left its keys
  //  undecoded -- the fine level of a chained call -- has them decoded by this pass.)
  return launch_csm_exact_score(job, plan);
}

int launch_csm_scores(const MatchJob &job, int32_t src, int32_t slot, int32_t origin_x, int32_t origin_y, int32_t *d_volume) {
  const GridLayout &L = *job.L;
  int rc = check_search(job.spec, L, job.search);
  if (rc) return rc;
  NHIP_REQUIRE(L.has_image, "csm_scores: the score volume comes from the kernel that performs every add, which reads the row-major "
               "image the grids were built without (NHIP_GRID_NO_IMAGE)");
  const StripKernels &K = strip_kernels(L);
  const hipStream_t s = job.stream;
  CsmParams P;
  fill_params(P, job, K);  // (the job's pair arrays, ids and keys are null: the one pair is the single_* fields below)
  P.volume = d_volume;
  P.n_pairs = 1;
  P.single_src = src;
  P.single_slot = slot;
  P.single_ox = origin_x;
  P.single_oy = origin_y;
  const int64_t blocks = (int64_t)P.n_theta * P.npbx * P.npby;
  hipLaunchKernelGGL(K.scores[P.dense], dim3((uint32_t)blocks), dim3(K.threads), 0, s, P);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
