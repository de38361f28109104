// nhip_host.h -- what the host units of the C ABI share (nhip_runtime, nhip_dropin and every nhip_host_*.hip): the pooled
// device buffer, the in-flight guard, the staged call of the handle forms, the phase clocks, the scan and grid handles.
// Host only: no kernel unit includes it.
#pragma once
#include <atomic>
#include <chrono>
#include <deque>
#include <mutex>

#include "nhip_common.h"

namespace nhip {

// ---- host phases of the handle API (nhip_host_phases; nhip_runtime.hip) ----
enum { PH_ALLOC = 0, PH_UPLOAD, PH_ENQUEUE, PH_WAIT, PH_DOWNLOAD, PH_FREE, PH_HOST, PH_COUNT };
struct PhaseClock {  // its lifetime is added to phase `id` of the calling thread
  int id;
  std::chrono::steady_clock::time_point t0;
  explicit PhaseClock(int i) : id(i), t0(std::chrono::steady_clock::now()) {}
  ~PhaseClock();
};
void phases_reset();

// ---- device buffers of the handle API (the pool behind them: nhip_runtime.hip) ----
struct InFlight {  // work this thread's call enqueued may still run: a DevBuf released meanwhile waits for the device first
  InFlight();
  static void done();  // (the caller has synchronised)
};

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  int device = -1;  // the device the memory lives on
  int alloc(size_t n);
  void free(uint64_t key = 0, uint64_t meta = 0);  // (key, meta: the contents stay known to the pool, see PoolEntry)
  void adopt(void *q, size_t n);                   // (a buffer pool_take_pair returned: filed under the current device)
  template <class T> T *as() const { return static_cast<T *>(p); }
  ~DevBuf() { free(); }
};
// the two buffers of one keyed release (metas `meta_a`, `meta_b`), if both are still in the pool
bool pool_take_pair(uint64_t meta_a, uint64_t meta_b, size_t need_a, size_t need_b, void **pa, size_t *ba, void **pb, size_t *bb);
extern std::atomic<uint64_t> g_pool_key;

// One call of a handle form (host arrays in, null stream, host arrays out): the device buffers it stages, its copies and
// the wait it owes.  Errors are sticky: after the first one every in / out / fetch does nothing and returns null, and the
// form asks ok() once before it launches, so no null pointer reaches a launcher.  A buffer's size, its copy's size and its
// element type come from one (T, count).
class Staged {
 public:
  Staged() = default;
  Staged(const Staged &) = delete;
  Staged &operator=(const Staged &) = delete;
  ~Staged();  // work enqueued and not waited for (an error path): waits for the device, then the buffers go back to the pool
  template <class T> T *out(size_t count) { return static_cast<T *>(stage(nullptr, count * sizeof(T))); }  // (0: a placeholder, not null)
  template <class T> T *inout(const T *host, size_t count) { return static_cast<T *>(stage(host, count * sizeof(T))); }
  template <class T> const T *in(const T *host, size_t count) { return inout(host, count); }  // (null host: nothing is copied)
  template <class T> void fetch(T *host, const T *dev, size_t count) { download(host, dev, count * sizeof(T)); }  // (null host: nothing)
  bool ok() const { return rc_ == NHIP_OK; }
  void launched(int rc);  // a launcher's return code: non-zero is the call's error; either way work may be in flight from here
  int finish();           // the first error, or NHIP_OK with the null stream drained (the downloads did that, if there were any)

 private:
  void *stage(const void *host, size_t bytes);
  void download(void *host, const void *dev, size_t bytes);
  std::deque<DevBuf> bufs_;  // (a deque: growing it moves no DevBuf)
  int rc_ = NHIP_OK;
  bool inflight_ = false;
};

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }  // (a: a power of two)

constexpr size_t STATS_WORDS = 8;  // a stats block: eight words (int64 in most units, int32 in vectorize)

}  // namespace nhip

// ---- the handles ----
struct nhip_scans {
  nhip::DevBuf xy, offsets;
  int32_t n_scans = 0;
  int64_t n_points = 0;
  std::vector<int32_t> h_offsets;
};

struct nhip_grids {
  nhip::DevBuf grids;
  nhip::DevBuf ws;         // the build's workspace: its tile list and line masks describe what `grids` holds
  uint64_t shape = 0;      // digest of (spec as built, targets): what a later build must equal to rebuild into these buffers
  bool dirty = false;      // something besides the build wrote into `grids` (a late skip-map build): contents no longer the list's
  bool rebuilt = false;    // this handle's build was an incremental rebuild into a kept pair
  nhip_grid_spec_t spec;
  nhip::GridLayout L;
  int32_t n = 0;
  std::mutex mu;  // (the late skip-map build, the late free-space trace)
  // the free-space check (nhip_csm_freespace): the scan behind every slot, whether the slots are submaps, and the free
  // planes, traced by the first check on the handle and kept with it
  std::vector<int32_t> target_ids;
  bool submaps = false, free_traced = false;
  nhip::DevBuf free_planes;
};

namespace nhip {

// 16-bit grids are built without skip maps unless their spec asks (only the 16-bit strip kernels read them).
// The first search on a handle whose plan takes those kernels builds them, once.  (nhip_host_csm.hip)
int ensure_skip_maps(const nhip_grids_t *grids, const MatchPlan &plan);
// the handle's spec as it is now (the flags may be written by a concurrent call's ensure_skip_maps: read under the same lock)
int spec_under_lock(nhip_grids_t *g, nhip_grid_spec_t *out);

// a job on scans and grids of the handle API: the five fields every such search takes from them; the rest by name, per call
inline MatchJob job_on(const DevBuf &xy, const DevBuf &offsets, const nhip_grids &g, const nhip_grid_spec_t &spec_now) {
  MatchJob job;
  job.xy = xy.as<const float>();
  job.offsets = offsets.as<const int32_t>();
  job.grids = g.grids.as<const uint8_t>();
  job.spec = &spec_now;
  job.L = &g.L;
  return job;
}

}  // namespace nhip
