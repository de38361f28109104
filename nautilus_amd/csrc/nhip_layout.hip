// nhip_layout.hip -- the tables of a grid spec and the arithmetic of the ABI that needs no device: slot layout, blur
// taps, quantiser thresholds, rotation tables, records to transforms, sums to scores, the robust loss' spec check.  Nothing
// here calls HIP.
#include <map>
#include <mutex>

#include "nhip_common.h"
#include "nhip_csm_shared.h"  // (the score gate's floor)
#include "nhip_loss_shared.h"  // (log1p_pinned: its host compilation, for nhip_loss_log1p_pinned)

namespace nhip {

// ---------------------------------------------------------------- spec tables (host)
// integer taps of the blur: round(16384 * g_i / sum g), i = -R .. R; returns their sum
static int64_t make_taps(double sigma, int32_t R, int32_t *taps) {
  double g[129], tot = 0.0;
  for (int i = -R; i <= R; i++) {
    g[i + R] = exp(-((double)i * (double)i) / (2.0 * sigma * sigma));
    tot += g[i + R];
  }
  int64_t K = 0;
  for (int i = 0; i <= 2 * R; i++) K += taps[i] = (int32_t)floor(16384.0 * g[i] / tot + 0.5);
  return K;
}

int make_layout(const nhip_grid_spec_t *spec, GridLayout *L) {
  NHIP_REQUIRE(spec != nullptr && L != nullptr, "grid spec: null pointer");
  NHIP_REQUIRE(spec->range > 0 && spec->res > 0, "grid spec: range and res must be > 0");
  NHIP_REQUIRE(spec->sigma > 0 && spec->sigma <= 16.0 / 3.0, "grid spec: sigma must be in (0, 5.33] cells");
  NHIP_REQUIRE(spec->floor_p > 0 && spec->floor_p < 1, "grid spec: floor_p must be in (0, 1)");
  NHIP_REQUIRE(spec->max_shift >= 0 && spec->max_shift <= 4096, "grid spec: max_shift out of range");
  NHIP_REQUIRE(spec->cell_bits == 0 || spec->cell_bits == 8 || spec->cell_bits == 16,
               "grid spec: cell_bits must be 8 or 16 (0 = 16), got %d", spec->cell_bits);
  NHIP_REQUIRE((spec->flags & ~(NHIP_GRID_SKIP_MAP | NHIP_GRID_NO_IMAGE)) == 0 && spec->reserved == 0,
               "grid spec: unknown flags %d / reserved %d", spec->flags, spec->reserved);
  NHIP_REQUIRE((spec->flags & (NHIP_GRID_SKIP_MAP | NHIP_GRID_NO_IMAGE)) != (NHIP_GRID_SKIP_MAP | NHIP_GRID_NO_IMAGE),
               "grid spec: a skip map (the every-add kernels') needs the image NHIP_GRID_NO_IMAGE leaves out");
  const double side = floor((spec->range * 2.0) / spec->res);  // cimg_debug.h:21-22
  NHIP_REQUIRE(side >= 1 && side <= GRID_MAX_SIDE, "grid spec: side %g out of range [1, %d]", side, GRID_MAX_SIDE);
  L->S = (int32_t)side;
  L->cb = spec->cell_bits == 8 ? 1 : 2;  // (0 = the default: 16-bit cells, in every struct of the ABI)
  L->levels = L->cb == 2 ? 65535 : 255;
  L->pad = ((2 * spec->max_shift + 16) + 3) & ~3;
  L->pitch = ((L->S + 2 * L->pad) * L->cb + 15) & ~15;
  L->R = (int32_t)ceil(3.0 * spec->sigma);
  L->plain_bytes = (int64_t)L->pitch * (int64_t)(L->S + 2 * L->pad);
  L->has_image = !(spec->flags & NHIP_GRID_NO_IMAGE);
  L->grid_bytes = L->has_image ? L->plain_bytes : 0;
  L->skip_bytes = L->has_image ? (((int64_t)skip_pitch(L->pitch) * (int64_t)(L->S + 2 * L->pad)) + 15) & ~15ll : 0;
  // pooled table: one byte per 8 x 8 stored cells, + BNB_MAX_NB rows / + BNB_MAX_NB + 5 columns of zeros so that a
  // window origin anywhere in the stored image can read its 11 x 16-byte rows without bounds checks
  L->pool_rows = (L->S + 2 * L->pad + BNB_B - 1) / BNB_B + BNB_MAX_NB + 1;
  L->pool_pitch = (((L->S + 2 * L->pad + BNB_B - 1) / BNB_B + BNB_MAX_NB + 5) + 15) & ~15;
  L->pool_bytes = (int64_t)L->pool_rows * L->pool_pitch;
  // second-level table: per 4 x 4 stored cells a PAIR of bytes {P4[i][j], P4[i + 1][j]} (the two sub-block rows of a
  // block in one read); a block's sub-blocks reach 2 * BNB_MAX_NB entries past the origin's, and a strip of three
  // blocks is read as 16 bytes from a 4-byte-aligned offset
  L->pool4_rows = (L->S + 2 * L->pad + BNB_B4 - 1) / BNB_B4 + 2 * BNB_MAX_NB + 2;
  L->pool4_pitch = ((2 * ((L->S + 2 * L->pad + BNB_B4 - 1) / BNB_B4 + 2 * BNB_MAX_NB + 2) + 16) + 15) & ~15;
  L->pool4_bytes = (int64_t)L->pool4_rows * L->pool4_pitch;
  // The matcher's planes behind the two tables are stored ONE CACHE LINE PER TILE (128 bytes): they must start on a line
  // boundary in EVERY slot, or each tile read touches two lines.  (Round 5 appended the hit raster, whose size is not a
  // multiple of 128: slots 1, 2, ... started 16, 32, ... bytes off a line, and the candidates kernel's L2 fetch went from 0.86
  // to 1.39 GB per 10,000 pairs -- profiles/r06_cand_traffic_bisect.txt.)  So the second table is padded to the next line
  // boundary of the slot here, and the raster -- the slot's last part -- below.
  L->skip_offset = L->grid_bytes;
  L->pool_offset = L->skip_offset + L->skip_bytes;
  L->pool4_offset = L->pool_offset + L->pool_bytes;
  L->pool4_bytes += (128 - ((L->pool4_offset + L->pool4_bytes) & 127)) & 127;
  L->hi_offset = L->pool4_offset + L->pool4_bytes;
  // 16-bit cells: the plane of their high bytes, one byte per cell at the 8-bit pitch.  The matcher sums exact 8 x 8
  // and 4 x 4 blocks on this plane at the cost of 8-bit cells (256 * sum(hi) + 255 * points bounds a pose's sum from
  // above) and reads 16-bit cells only for the poses that bound still admits (nhip_bnb_exact.h refine16)
  // (8-bit cells: the same two tiled copies hold the cells themselves -- the image's bytes)
  L->hi_pitch = ((L->S + 2 * L->pad) + 15) & ~15;
  L->hi_tpr = L->hi_pitch / 16 + 1;  // (+ 1: the shifted copy's last tile)
  L->hi_copy_bytes = (int64_t)((L->S + 2 * L->pad + 7) / 8) * L->hi_tpr * (int64_t)HI_TILE_BYTES;
  L->t16_tpr = L->cb == 2 ? L->hi_pitch / 8 : 0;
  L->t16_bytes = (int64_t)((L->S + 2 * L->pad + 7) / 8) * L->t16_tpr * (int64_t)HI_TILE_BYTES;
  L->hi_bytes = 2 * L->hi_copy_bytes + L->t16_bytes;  // (the matcher's private planes, all three)
  L->t16_offset = L->hi_offset + 2 * L->hi_copy_bytes;
  L->hits_offset = L->hi_offset + L->hi_bytes;
  // the hit raster, one bit per cell + a zero border of HIT_PAD cells: bit rows of whole dwords
  L->hits_pitch = ((L->S + 2 * HIT_PAD + 31) / 32) * 4;
  L->hits_bytes = (((int64_t)L->hits_pitch * (L->S + 2 * HIT_PAD) + 8) + 15) & ~15ll;  // (+ 8: a row's last 64-bit window)
  L->hits_bytes += (128 - ((L->hits_offset + L->hits_bytes) & 127)) & 127;  // (every slot starts on a line boundary: see pool4_bytes above)
  L->slot_bytes = L->hits_offset + L->hits_bytes;
  L->Lf = log(spec->floor_p);
  L->step = -L->Lf / (double)L->levels;
  int32_t taps[129];
  L->K = make_taps(spec->sigma, L->R, taps);
  return NHIP_OK;
}

// The quantiser of the spec, evaluated directly (used only to build the threshold table).
static uint32_t quantise_direct(uint64_t V, int64_t K, double floor_p, int32_t levels) {
  double v = (double)V / ((double)K * (double)K);
  if (v < floor_p) v = floor_p;
  const double Lf = log(floor_p);
  const double step = -Lf / (double)levels;
  double q = floor((log(v) - Lf) / step + 0.5);
  if (q < 0.0) q = 0.0;
  if (q > (double)levels) q = (double)levels;
  return (uint32_t)q;
}

// thr[k] = smallest integer V in [0, K*K] whose quantised value is >= k (0xffffffff: level never reached).
// q is non-decreasing in V, so a binary search per level is exact; it starts from a bracket around the
// closed-form inverse so that the 65535 levels of the 16-bit table cost a few log() calls each.
static void make_thresholds(int64_t K, double floor_p, int32_t levels, uint32_t *thr) {
  const uint64_t vmax = (uint64_t)K * (uint64_t)K;
  const double Lf = log(floor_p), step = -Lf / (double)levels;
  auto q = [&](uint64_t V) { return quantise_direct(V, K, floor_p, levels); };
  const uint32_t q0 = q(0), qmax = q(vmax);
  thr[0] = 0;
  for (int32_t k = 1; k <= levels; k++) {
    if (qmax < (uint32_t)k) { thr[k] = 0xffffffffu; continue; }
    if (q0 >= (uint32_t)k) { thr[k] = 0; continue; }
    // invariant: q(lo) < k <= q(hi)
    uint64_t lo = 0, hi = vmax;
    const double est = (double)vmax * exp(Lf + ((double)k - 0.5) * step);
    if (est > 2.0 && est < (double)vmax) {
      const uint64_t e = (uint64_t)est, w = e / 1000000 + 2;  // ~1e-6 relative bracket
      const uint64_t a = e > w ? e - w : 0, b = e + w < vmax ? e + w : vmax;
      if (q(a) < (uint32_t)k) lo = a;
      if (q(b) >= (uint32_t)k) hi = b;
    }
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (q(mid) >= (uint32_t)k) hi = mid; else lo = mid;
    }
    thr[k] = (uint32_t)hi;
  }
}

int make_tables(const nhip_grid_spec_t *spec, const GridLayout &L, GridTables *T) {
  memset(T, 0, sizeof(*T));
  make_taps(spec->sigma, L.R, T->taps);
  if (L.cb == 1) {
    make_thresholds(L.K, spec->floor_p, 255, T->thr);
    return NHIP_OK;
  }
  // 16-bit cells: 65536 entries, computed once per (tap sum, floor) and kept for the life of the process
  static std::mutex mu;
  static std::map<std::pair<int64_t, double>, std::vector<uint32_t>> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto &v = cache[{L.K, spec->floor_p}];
  if (v.empty()) {
    v.resize(65536);
    make_thresholds(L.K, spec->floor_p, 65535, v.data());
  }
  T->thr16 = v.data();
  return NHIP_OK;
}

// ---------------------------------------------------------------- the robust loss' spec (host)
// the accepted ranges of include/nautilus_hip.h
int loss_spec_check(const nhip_loss_spec_t *loss, const char *who) {
  NHIP_REQUIRE(loss, "%s: null loss spec", who);
  NHIP_REQUIRE(loss->kind >= NHIP_LOSS_NONE && loss->kind <= NHIP_LOSS_CAUCHY, "%s: loss kind %d outside 0..3", who, loss->kind);
  NHIP_REQUIRE(loss->flags == 0, "%s: loss flags %d: none is defined", who, loss->flags);
  NHIP_REQUIRE(loss->kind == NHIP_LOSS_NONE || (std::isfinite(loss->scale) && loss->scale > 0.0),
               "%s: loss scale %g must be finite and > 0", who, loss->scale);
  return NHIP_OK;
}

// ---------------------------------------------------------------- relative-pose factors: their arguments (host)
int relpose_args_check(const void *z, const void *info, const void *pose_i, const void *pose_j, int32_t n_factors,
                       const void *poses, int32_t n_poses, const void *out, const char *who) {
  NHIP_REQUIRE(n_factors >= 0 && n_poses >= 0, "%s: negative size (n_factors %d, n_poses %d)", who, n_factors, n_poses);
  NHIP_REQUIRE(z && info && pose_i && pose_j && poses && out, "%s: null pointer", who);
  return NHIP_OK;
}

}  // namespace nhip

using namespace nhip;

extern "C" {

int nhip_loss_log1p_pinned(const double *x, int64_t n, double *out) {
  NHIP_REQUIRE(n >= 0 && (n == 0 || (x && out)), "loss_log1p_pinned: bad arguments");
  for (int64_t i = 0; i < n; i++) out[i] = log1p_pinned(x[i]);
  return NHIP_OK;
}

int nhip_relpose_information(const nhip_refined_t *refined, int32_t n, double sigma_m, double wt, double wr, double *info,
                             uint8_t *from_icp) {
  NHIP_REQUIRE(n >= 0, "relpose_information: negative size %d", n);
  NHIP_REQUIRE(std::isfinite(sigma_m) && sigma_m > 0.0, "relpose_information: sigma_m %g must be finite and > 0", sigma_m);
  NHIP_REQUIRE(std::isfinite(wt) && std::isfinite(wr), "relpose_information: weights (%g, %g) must be finite", wt, wr);
  NHIP_REQUIRE(n == 0 || info, "relpose_information: null info");
  const double inv = 1.0 / (sigma_m * sigma_m), tt = wt * wt, rr = wr * wr;
  for (int32_t k = 0; k < n; k++) {
    double *L = info + 6 * (size_t)k;
    const bool icp = refined && (refined[k].flags & ~NHIP_REFINE_NOT_CONVERGED) == 0u;
    if (icp) {
      for (int q = 0; q < 6; q++) L[q] = refined[k].info[q] * inv;
    } else {
      L[0] = tt, L[1] = 0.0, L[2] = 0.0, L[3] = tt, L[4] = 0.0, L[5] = rr;
    }
    if (from_icp) from_icp[k] = icp ? 1 : 0;
  }
  return NHIP_OK;
}

int nhip_grid_layout(const nhip_grid_spec_t *spec, nhip_grid_layout_t *out) {
  GridLayout L;
  int rc = make_layout(spec, &L);
  if (rc) return rc;
  NHIP_REQUIRE(out != nullptr, "grid_layout: null out");
  out->side = L.S;
  out->pad = L.pad;
  out->pitch = L.pitch;
  out->rows = L.S + 2 * L.pad;
  out->blur_radius = L.R;
  out->cell_bytes = L.cb;
  out->tap_sum = L.K;
  out->grid_bytes = L.grid_bytes;
  out->score_floor = L.Lf;
  out->score_step = L.step;
  out->skip_bytes = L.skip_bytes;
  out->slot_bytes = L.slot_bytes;
  out->pool_bytes = L.pool_bytes;
  out->pool_pitch = L.pool_pitch;
  out->pool_rows = L.pool_rows;
  out->pool4_bytes = L.pool4_bytes;
  out->pool4_pitch = L.pool4_pitch;
  out->pool4_rows = L.pool4_rows;
  out->hi_bytes = L.hi_bytes;
  out->hi_pitch = L.hi_pitch;
  out->hits_pitch = L.hits_pitch;
  out->hits_bytes = L.hits_bytes;
  return NHIP_OK;
}

int64_t nhip_grids_bytes(const nhip_grid_spec_t *spec, int64_t n_grids) {
  GridLayout L;
  if (make_layout(spec, &L)) return -1;
  return n_grids * L.slot_bytes + 256;
}

int64_t nhip_grid_workspace_bytes(const nhip_grid_spec_t *spec, int32_t chunk) {
  GridLayout L;
  if (make_layout(spec, &L)) return -1;
  if (chunk < 1) chunk = 1;
  // header | [16-bit threshold table] | tile occupancy | tile list
  return GRID_WS_HEADER + (L.cb == 2 ? GRID_WS_THR16 : 0) + 4 + (int64_t)chunk * grid_ws_per_target(L.S);
}

int nhip_grid_tables(const nhip_grid_spec_t *spec, int32_t *taps, uint32_t *thresholds) {
  GridLayout L;
  int rc = make_layout(spec, &L);
  if (rc) return rc;
  GridTables T;
  rc = make_tables(spec, L, &T);
  if (rc) return rc;
  if (taps) memcpy(taps, T.taps, sizeof(int32_t) * (2 * L.R + 1));
  if (thresholds && L.cb == 1) memcpy(thresholds, T.thr, sizeof(T.thr));
  if (thresholds && L.cb == 2) memcpy(thresholds, T.thr16, sizeof(uint32_t) * 65536);
  return NHIP_OK;
}

int nhip_csm_rot0(const double *rot_a, const double *rot_b, int32_t n, double *cs_out) {
  NHIP_REQUIRE(rot_a && cs_out && n >= 0, "csm_rot0: bad arguments");
  for (int32_t i = 0; i < n; i++) {
    // math_util.h:81-89: AngleDiff(a0, a1) = AngleMod(a0 - a1), AngleMod: a -= 2pi*rint(a / 2pi)
    double a = rot_a[i] - (rot_b ? rot_b[i] : 0.0);
    a -= (2.0 * M_PI) * rint(a / (2.0 * M_PI));
    cs_out[2 * i] = cos(a);
    cs_out[2 * i + 1] = sin(a);
  }
  return NHIP_OK;
}

int nhip_csm_delta_table(const nhip_search_t *search, double *cs_out) {
  NHIP_REQUIRE(search && cs_out && search->n_theta >= 1, "csm_delta_table: bad arguments");
  for (int32_t k = 0; k < search->n_theta; k++) {
    const double d = (double)(k - (search->n_theta - 1) / 2) * search->theta_step;
    cs_out[2 * k] = cos(d);
    cs_out[2 * k + 1] = sin(d);
  }
  return NHIP_OK;
}

int nhip_match_to_transform(const nhip_match_t *m, const nhip_grid_spec_t *spec,
                            const nhip_search_t *search, double theta0, int32_t origin_x,
                            int32_t origin_y, float *tx, float *ty, float *theta) {
  NHIP_REQUIRE(m && spec && search, "match_to_transform: null argument");
  if (tx) *tx = (float)((double)(origin_x + m->ix - (search->nx - 1) / 2) * spec->res);
  if (ty) *ty = (float)((double)(origin_y + m->iy - (search->ny - 1) / 2) * spec->res);
  if (theta) *theta = (float)(theta0 + (double)(m->itheta - (search->n_theta - 1) / 2) * search->theta_step);
  return NHIP_OK;
}

double nhip_score_from_sum(const nhip_grid_spec_t *spec, int64_t sum, int32_t n_points) {
  const double Lf = log(spec->floor_p), step = -Lf / (spec->cell_bits == 8 ? 255.0 : 65535.0);
  if (n_points <= 0) return Lf;
  const double t = step * (double)sum;
  const double u = t / (double)n_points;
  return Lf + u;
}

int nhip_csm_gate_floor(const nhip_grid_spec_t *spec, double min_score, int32_t n_points, int32_t *floor_sum) {
  NHIP_REQUIRE(spec && floor_sum, "csm_gate_floor: null argument");
  NHIP_REQUIRE(!std::isnan(min_score), "csm_gate_floor: min_score is NaN");
  NHIP_REQUIRE(n_points >= 0, "csm_gate_floor: n_points %d < 0", n_points);
  GridLayout L;
  const int rc = make_layout(spec, &L);
  if (rc) return rc;
  *floor_sum = gate_floor(ScoreGate{min_score, L.Lf, L.step}, n_points);
  return NHIP_OK;
}

}  // extern "C"
