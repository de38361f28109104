// nhip_runtime.hip -- what every host unit of libnautilus_hip stands on: the error message, the device status words, the
// in-stream timers, the host phase clocks, the device-memory pool behind DevBuf, pinned host memory.
#include <atomic>
#include <cstdarg>
#include <map>
#include <mutex>

#include "nhip_common.h"
#include "nhip_host.h"

namespace nhip {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
  set_error("HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
  return NHIP_ERR_HIP;
}

int require_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device visible (hipGetDeviceCount -> %d, n = %d): this library has no CPU path",
              (int)e, n);
    return NHIP_ERR_NODEV;
  }
  return NHIP_OK;
}

// The status words of a device (nhip_common.h, "ids that live in device memory"): 16 bytes of device memory per device,
// kept to the end of the process.  They are allocated and zeroed by dev_status_prepare() -- called from nhip_init (the
// current device) and nhip_set_device, i.e. OUTSIDE any launch path -- so that dev_status(), which every `_dev` launcher
// calls, is a lookup: no hipMalloc, no null-stream memset, nothing a stream capture could trip over.  A process that hands
// the library a device it never named to nhip_init / nhip_set_device gets the words on that device's first launch (the
// lazy path below; it synchronises once, and must not be the first thing inside a capture: include/nautilus_hip.h says so).
namespace {
constexpr int MAX_DEV = 64;
std::mutex g_status_mu;
std::atomic<uint32_t *> g_status_words[MAX_DEV];
}  // namespace

uint32_t *dev_status_prepare(int dev) {
  if (dev < 0 || dev >= MAX_DEV) return nullptr;
  if (uint32_t *w = g_status_words[dev].load(std::memory_order_acquire)) return w;
  std::lock_guard<std::mutex> lock(g_status_mu);
  if (uint32_t *w = g_status_words[dev].load(std::memory_order_acquire)) return w;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (cur != dev && hipSetDevice(dev) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  void *p = nullptr;
  bool ok = hipMalloc(&p, sizeof(uint32_t) * DEV_STATUS_WORDS) == hipSuccess;
  if (ok && hipMemset(p, 0, sizeof(uint32_t) * DEV_STATUS_WORDS) != hipSuccess) {
    (void)hipFree(p);  // (not leaked, and not retried with the same pointer)
    ok = false;
  }
  if (!ok) (void)hipGetLastError();
  if (cur != dev) (void)hipSetDevice(cur);
  if (!ok) return nullptr;
  g_status_words[dev].store(static_cast<uint32_t *>(p), std::memory_order_release);
  return static_cast<uint32_t *>(p);
}

uint32_t *dev_status() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (uint32_t *w = g_status_words[dev].load(std::memory_order_acquire)) return w;
  return dev_status_prepare(dev);
}

const char *tunable(const char *name) {
  static std::once_flag once;
  static bool on = false;
  std::call_once(once, [] {
    const char *e = getenv("NHIP_TUNABLES");
    on = e && e[0] == '1';
  });
  return on ? getenv(name) : nullptr;
}

// ---------------------------------------------------------------- in-stream timing
namespace {
struct TimerSlot {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  hipEvent_t open = nullptr;
};
std::mutex g_tmu;
bool g_timing = false;
TimerSlot g_slots[NHIP_TIMER_COUNT];
}  // namespace

void timer_begin(int id, hipStream_t s) {
  if (!g_timing) return;
  std::lock_guard<std::mutex> lk(g_tmu);
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_slots[id].open = e;
}

void timer_end(int id, hipStream_t s) {
  if (!g_timing) return;
  std::lock_guard<std::mutex> lk(g_tmu);
  if (!g_slots[id].open) return;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  g_slots[id].ev.emplace_back(g_slots[id].open, e);
  g_slots[id].open = nullptr;
}

// ---------------------------------------------------------------- host phases of the handle API
// Wall-clock seconds of the calling thread's LAST handle-API call (nhip_scans_upload, nhip_grids_build, nhip_csm_match,
// the *_free calls), by what the host was waiting for: nhip_host_phases().  Round 4's bench saw one call in five of the
// host-buffer route take 4 s instead of 12 ms and could not say where (a median hid it); the clocks cost two
// steady_clock reads per phase.
static thread_local double t_phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
PhaseClock::~PhaseClock() { t_phase[id] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
void phases_reset() {
  for (double &v : t_phase) v = 0.0;
}

// ---------------------------------------------------------------- device buffers of the handle API
// The handle entry points own their device memory and used to hipMalloc / hipFree it per call.  Measured in round 5
// (tools/r05_host_api_stall.py, profiles/r05_host_api_stall.txt): on a quiet device the pair costs microseconds, but
// hipFree is a device-wide synchronisation whose cost is the driver's -- 0.2 to 8 ms per nhip_csm_match call for its 328 MB
// of workspace, and 0.33 s PER hipFree of the 12 GB of tables for seconds after another client of the process (torch's
// caching allocator) had released 130 GB; round 4's bench saw one host-buffer call in five take 4 s.  So released buffers
// are kept, per device, up to a byte cap (nhip_device_pool_configure; least recently released out first) and handed to
// the next allocation they fit (at most twice the size asked for): a loop of build / match / free touches the driver's
// allocator once.  Contents are never assumed -- every user initialises what it reads -- with one exception, stated on the
// entries themselves: a table buffer and its build workspace released together (PoolEntry::key).
namespace {
struct PoolEntry {
  void *p;
  size_t bytes;
  int device;
  // A table buffer and the workspace of the build that filled it may come back TOGETHER with their contents known: both carry
  // the key of that release (0: contents unknown) and a digest of (spec, targets, which of the two).  While both are still in
  // the pool nobody has written to either, so a build of the same shape takes the pair and rebuilds incrementally -- it clears
  // the lines the previous build wrote instead of zero-filling gigabytes (pool_take_pair).
  uint64_t key = 0, meta = 0;
};
std::mutex g_pool_mu;
std::vector<PoolEntry> &g_pool = *new std::vector<PoolEntry>();  // oldest first (never destroyed: see the drop-in cache, nhip_dropin.hip)
// PER DEVICE.  4 GB by default: enough for the workspace of a 10,000-pair match (0.33 GB), the tables of ~450 targets and the
// small per-call buffers -- what a drop-in host that called the library once can defend holding.  A host that cycles
// larger tables (bench.py's host-buffer leg: 8.3 GB) raises it with nhip_device_pool_configure.
int64_t g_pool_cap = 4ll << 30;
constexpr size_t POOL_MAX_ENTRIES = 32;

int current_device() {
  int d = -1;
  if (hipGetDevice(&d) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return d;
}
void *pool_take(size_t n, size_t *got) {
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_pool_mu);
  // best fit; a buffer whose contents are known (half of a kept pair, see PoolEntry) only when nothing else fits
  size_t best = g_pool.size();
  for (int keyed = 0; keyed < 2 && best == g_pool.size(); keyed++)
    for (size_t i = 0; i < g_pool.size(); i++)
      if (g_pool[i].device == dev && (g_pool[i].key != 0) == (keyed == 1) && g_pool[i].bytes >= n &&
          g_pool[i].bytes <= 2 * n + (1u << 20) && (best == g_pool.size() || g_pool[i].bytes < g_pool[best].bytes))
        best = i;
  if (best == g_pool.size()) return nullptr;
  void *p = g_pool[best].p;
  *got = g_pool[best].bytes;
  g_pool.erase(g_pool.begin() + (long)best);
  return p;
}
// true: the pool keeps the buffer; `evict` receives what it lets go of for it (freed by the caller, outside the lock)
// `dev`: the device the buffer was ALLOCATED on (DevBuf records it) -- not the device that happens to be current when it
// is released: a handle built on device 0 and freed after nhip_set_device(1) stays a device-0 buffer.  Cap and entry limit
// are per device: releases on one GPU never evict what another GPU's callers keep.
bool pool_put(void *p, size_t bytes, int dev, std::vector<void *> *evict, uint64_t key = 0, uint64_t meta = 0) {
  std::lock_guard<std::mutex> lock(g_pool_mu);
  if (dev < 0 || (int64_t)bytes > g_pool_cap) return false;
  g_pool.push_back({p, bytes, dev, key, meta});
  int64_t tot = 0;
  size_t cnt = 0;
  for (auto &e : g_pool)
    if (e.device == dev) {
      tot += (int64_t)e.bytes;
      cnt++;
    }
  for (size_t i = 0; i < g_pool.size() && (tot > g_pool_cap || cnt > POOL_MAX_ENTRIES);) {
    if (g_pool[i].device != dev) {
      i++;
      continue;
    }
    tot -= (int64_t)g_pool[i].bytes;  // (oldest of this device first)
    cnt--;
    evict->push_back(g_pool[i].p);
    g_pool.erase(g_pool.begin() + (long)i);
  }
  return true;
}
void pool_drain(std::vector<void *> *out, int device /* -1: every device */) {
  std::lock_guard<std::mutex> lock(g_pool_mu);
  for (size_t i = 0; i < g_pool.size();)
    if (device < 0 || g_pool[i].device == device) {
      out->push_back(g_pool[i].p);
      g_pool.erase(g_pool.begin() + (long)i);
    } else {
      i++;
    }
}
}  // namespace

bool pool_take_pair(uint64_t meta_a, uint64_t meta_b, size_t need_a, size_t need_b, void **pa, size_t *ba, void **pb, size_t *bb) {
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_pool_mu);
  for (size_t i = g_pool.size(); i-- > 0;) {  // (newest first)
    if (g_pool[i].device != dev || g_pool[i].key == 0 || g_pool[i].meta != meta_a || g_pool[i].bytes < need_a) continue;
    for (size_t j = 0; j < g_pool.size(); j++) {
      if (j == i || g_pool[j].device != dev || g_pool[j].key != g_pool[i].key || g_pool[j].meta != meta_b || g_pool[j].bytes < need_b)
        continue;
      *pa = g_pool[i].p; *ba = g_pool[i].bytes;
      *pb = g_pool[j].p; *bb = g_pool[j].bytes;
      g_pool.erase(g_pool.begin() + (long)(i > j ? i : j));
      g_pool.erase(g_pool.begin() + (long)(i > j ? j : i));
      return true;
    }
  }
  return false;
}
std::atomic<uint64_t> g_pool_key{1};

// Work this thread's current handle call has enqueued may still be running: set by the entry points that launch kernels
// on buffers they own (InFlight), cleared once they have synchronised.  DevBuf::free used to be a hipFree -- an implicit
// device-wide synchronisation -- and is now a hand-over to the pool: on an error path (a failed launch after earlier ones
// were enqueued, a failed round of the split form with the helper stream still busy) the buffers would return to the pool
// while kernels still read or write them.  So the first release under the flag waits for the device.
static thread_local bool t_inflight = false;
InFlight::InFlight() { t_inflight = true; }
void InFlight::done() { t_inflight = false; }

int DevBuf::alloc(size_t n) {
  free();
  if (n == 0) n = 16;
  PhaseClock pc(PH_ALLOC);
  size_t got = 0;
  device = current_device();
  if (void *q = pool_take(n, &got)) {
    p = q;
    bytes = got;
    return NHIP_OK;
  }
  hipError_t e = hipMalloc(&p, n);
  if (e != hipSuccess) {  // (what the pool holds may be what is missing: let go of it and ask once more)
    (void)hipGetLastError();
    std::vector<void *> drop;
    pool_drain(&drop, current_device());
    for (void *d : drop) (void)hipFree(d);
    e = drop.empty() ? e : hipMalloc(&p, n);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    p = nullptr;
    set_error("hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
    return NHIP_ERR_ALLOC;
  }
  bytes = n;
  return NHIP_OK;
}
void DevBuf::free(uint64_t key, uint64_t meta) {
  if (p) {
    PhaseClock pc(PH_FREE);
    if (t_inflight) {  // an error path: nothing that was enqueued may outlive its buffers' release
      (void)hipDeviceSynchronize();
      (void)hipGetLastError();
      t_inflight = false;
    }
    std::vector<void *> evict;
    if (!pool_put(p, bytes, device, &evict, key, meta)) (void)hipFree(p);
    for (void *d : evict) (void)hipFree(d);
  }
  p = nullptr;
  bytes = 0;
}
void DevBuf::adopt(void *q, size_t n) {
  free();
  p = q;
  bytes = n;
  device = current_device();
}

// ---------------------------------------------------------------- the staged call of the handle forms
// The call keeps its own in-flight state: it does not lean on the thread-local flag above, on where the form declares it,
// or on which buffer is released first.  The destructor's body runs before any member is destroyed.
Staged::~Staged() {
  if (inflight_) {
    PhaseClock pc(PH_FREE);  // (where DevBuf::free counts the same wait)
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
  }
}
void *Staged::stage(const void *host, size_t bytes) {
  if (rc_) return nullptr;
  bufs_.emplace_back();
  DevBuf &d = bufs_.back();
  if ((rc_ = d.alloc(bytes))) return nullptr;
  if (host && bytes) {
    hipError_t e = hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      rc_ = hip_fail(e, "hipMemcpy, host to device", __FILE__, __LINE__);
      return nullptr;
    }
  }
  return d.p;
}
void Staged::download(void *host, const void *dev, size_t bytes) {
  if (rc_ || !host || !dev || !bytes) return;
  hipError_t e = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    rc_ = hip_fail(e, "hipMemcpy, device to host", __FILE__, __LINE__);
    return;
  }
  inflight_ = false;  // (a blocking copy on the null stream: what the call enqueued there has finished)
}
void Staged::launched(int rc) {
  inflight_ = true;  // (a launcher that fails may have enqueued part of its work)
  if (!rc_) rc_ = rc;
}
int Staged::finish() {
  if (!rc_ && inflight_) {
    hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return rc_ = hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    inflight_ = false;
  }
  return rc_;
}

}  // namespace nhip

using namespace nhip;

extern "C" {

const char *nhip_last_error(void) { return g_err.c_str(); }
const char *nhip_version(void) { return "nautilus_hip 0.1 (gfx950)"; }

int nhip_init(int *n_devices) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  if (n_devices) *n_devices = n;
  if (n <= 0) {
    set_error("no HIP device visible");
    return NHIP_ERR_NODEV;
  }
  int cur = 0;
  if (hipGetDevice(&cur) == hipSuccess) {
    (void)dev_status_prepare(cur);  // (the other devices' words: nhip_set_device, before that device's first launch)
  } else {
    (void)hipGetLastError();
  }
  return NHIP_OK;
}

int nhip_set_device(int device) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_TRY_HIP(hipSetDevice(device));
  (void)dev_status_prepare(device);
  return NHIP_OK;
}

int nhip_dev_status(void *stream, int32_t info[4]) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_TRY_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  uint32_t w[DEV_STATUS_WORDS] = {0u, 0u, 0u, 0u};
  uint32_t *st = dev_status();
  if (st) NHIP_TRY_HIP(hipMemcpy(w, st, sizeof(w), hipMemcpyDeviceToHost));
  if (info)
    for (int i = 0; i < 4; i++) info[i] = (int32_t)w[i];
  if (w[0] == 0u) return NHIP_OK;
  // cleared in the order of the stream that was asked about (a null-stream memset would race with kernels that are
  // flagging ids on other streams); the words are ONE set per device: see the header on what that means for several clients
  NHIP_TRY_HIP(hipMemsetAsync(st, 0, sizeof(w), static_cast<hipStream_t>(stream)));
  NHIP_TRY_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  const char *what = w[1] == BAD_TARGET_ID  ? "target scan id (nhip_grid_build_dev / nhip_grid_rebuild_dev: d_target_ids)"
                     : w[1] == BAD_PAIR_SRC  ? "source scan id (nhip_csm_match_dev: d_pair_src)"
                     : w[1] == BAD_PAIR_SLOT ? "grid slot (nhip_csm_match_dev: d_pair_slot)"
                     : w[1] == BAD_BLOCK_ID  ? "block id (d_corr_block)"
                     : w[1] == BAD_POSE_ID   ? "pose index (d_block_src / d_block_tgt / pose arrays)"
                     : w[1] == BAD_SCAN_ID   ? "scan id (d_block_src / d_block_tgt of the correspondence search)"
                     : w[1] == BAD_FEATURE_IDX   ? "feature index (nhip_features_pack_dev: d_idx)"
                     : w[1] == BAD_FEATURE_COUNT ? "feature count (nhip_features_pack_dev: d_count)"
                     : w[1] == BAD_SCAN_OFFSETS  ? "scan offset (nhip_normals_estimate_dev: d_offsets)"
                     : w[1] == BAD_MEMBER_ID     ? "member scan id (nhip_submaps_gather_dev: d_member_scan)"
                     : w[1] == BAD_SUBMAP_CAPACITY ? "merged point count (nhip_submaps_gather_dev: more than out_capacity; index = n_targets)"
                     : w[1] == BAD_CONTRIB_ID    ? "contributor id (nhip_bsr_assemble_dev: d_contrib; index = the block)"
                     : w[1] == BAD_BLOCK_COLUMN  ? "block column (nhip_bsr_assemble_dev / nhip_bsr_pcg_dev: d_col; index = the block)"
                     : w[1] == BAD_SYSTEM_ID     ? "gauge or right-hand-side index (nhip_bsr_pcg_columns_dev: d_gauge / d_rhs_index; index = the system)"
                     : w[1] == BAD_MAP_SCAN_OFFSETS ? "scan offset (nhip_vectorize_dev / nhip_occupancy_dev / nhip_place_describe_dev / nhip_transient_filter_dev: d_offsets)"
                     : w[1] == BAD_PLACE_ID ? "scan id (nhip_place_match_dev / nhip_place_seq_match_dev: d_ids)"
                     : w[1] == BAD_FREESPACE_PAIR ? "source scan, grid slot or record index of a pair (nhip_freespace_check_dev; index = the pair)"
                     : w[1] == BAD_MAPWIN_CELLS ? "occupied-cell count beyond max_cells (nhip_mapwin_cells_dev; index = height) or row_ptr entry that is not a row (nhip_mapwin_gather_dev; index = the map row)"
                     : w[1] == BAD_MAPWIN_POINTS ? "window point count (nhip_mapwin_gather_dev: more than out_capacity; index = n_queries)"
                     : w[1] == BAD_RANGESIG ? "anchor count beyond max_anchors (nhip_rangesig_anchors_dev; index = max_anchors) or ray-table entry that is not a ray (nhip_rangesig_map_dev; index = the ray)"
                     : w[1] == BAD_REFINE_ID ? "source or target scan id of a pair (nhip_refine_icp_dev: d_pair_src / d_pair_tgt; index = the pair)"
                                             : "id";
  set_error("an id read from device memory was out of range: %s = %d at index %d (kinds seen since the last check: 0x%x); "
            "the kernels treated every such entry as empty", what, (int32_t)w[2], (int32_t)w[3], w[0]);
  return NHIP_ERR_ARG;
}

int nhip_device_pool_configure(int64_t max_bytes) {
  NHIP_REQUIRE(max_bytes >= 0, "device_pool_configure: negative size");
  std::vector<void *> drop;
  {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    g_pool_cap = max_bytes;
    std::map<int, int64_t> tot;
    for (auto &e : g_pool) tot[e.device] += (int64_t)e.bytes;
    for (size_t i = 0; i < g_pool.size();) {  // (oldest first, each device against the cap on its own)
      if (tot[g_pool[i].device] > g_pool_cap) {
        tot[g_pool[i].device] -= (int64_t)g_pool[i].bytes;
        drop.push_back(g_pool[i].p);
        g_pool.erase(g_pool.begin() + (long)i);
      } else {
        i++;
      }
    }
  }
  for (void *d : drop) (void)hipFree(d);
  return NHIP_OK;
}

int nhip_device_pool_release(void) {
  std::vector<void *> drop;
  pool_drain(&drop, -1);
  for (void *d : drop) (void)hipFree(d);
  return NHIP_OK;
}

int nhip_device_pool_stats(int64_t *entries, int64_t *bytes) {
  std::lock_guard<std::mutex> lock(g_pool_mu);
  int64_t tot = 0;
  for (auto &e : g_pool) tot += (int64_t)e.bytes;
  if (entries) *entries = (int64_t)g_pool.size();
  if (bytes) *bytes = tot;
  return NHIP_OK;
}

int nhip_host_phases(double out[8]) {
  NHIP_REQUIRE(out != nullptr, "host_phases: null out");
  for (int i = 0; i < 8; i++) out[i] = t_phase[i];
  return NHIP_OK;
}

int nhip_host_alloc(size_t bytes, void **out) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(out, "host_alloc: null out");
  *out = nullptr;
  hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
  if (e != hipSuccess) {
    *out = nullptr;
    set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return NHIP_ERR_ALLOC;
  }
  return NHIP_OK;
}

int nhip_host_free(void *p) {
  if (p) NHIP_TRY_HIP(hipHostFree(p));
  return NHIP_OK;
}

// ---------------------------------------------------------------- timing
int nhip_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_tmu);
  g_timing = on != 0;
  return NHIP_OK;
}

int nhip_timing_reset(void) {
  std::lock_guard<std::mutex> lk(g_tmu);
  for (auto &s : g_slots) {
    for (auto &p : s.ev) {
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
    s.ev.clear();
    if (s.open) (void)hipEventDestroy(s.open);
    s.open = nullptr;
  }
  return NHIP_OK;
}

int nhip_timing_get(int id, double *total_ms, int32_t *launches) {
  NHIP_REQUIRE(id >= 0 && id < NHIP_TIMER_COUNT, "timing_get: bad id %d", id);
  std::lock_guard<std::mutex> lk(g_tmu);
  double tot = 0.0;
  for (auto &p : g_slots[id].ev) {
    NHIP_TRY_HIP(hipEventSynchronize(p.second));
    float ms = 0.f;
    NHIP_TRY_HIP(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (int32_t)g_slots[id].ev.size();
  return NHIP_OK;
}

}  // extern "C"
