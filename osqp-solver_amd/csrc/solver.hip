// solver.hip -- C-ABI (include/mi_osqp.h) over host_core + kernels.
//
// setup(): host analysis + Ruiz scaling + KKT + LDL' per QP (rows E1-E5), upload
// in tile-interleaved, schedule-ordered layout.  solve(): the whole ADMM loop
// runs inside admm_kernel; the host only reacts to "rho changed" requests
// (row E13: numeric refactor on the host, first version) and reads statuses.
// There is NO CPU solve path: without a gfx950 device setup returns
// MI_OSQP_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/mi_osqp.h"
#include "device_types.h"
#include "host_core.hpp"
#include "sched_format.h"

using namespace miosqp;
static_assert((int)kIterStreamed == RF_FORM_NONE && (int)kIterDeepRing == RF_FORM_DEEP_RING && (int)kIterLongHead == RF_FORM_LONG_HEAD, "iterate_form returns RF_FORM_*");

static thread_local std::string g_last_error;

#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    if (getenv("MI_OSQP_DEBUG_HIP")) {                                                   \
      hipError_t _s = hipGetLastError();                                                 \
      if (_s != hipSuccess) fprintf(stderr, "[mi_osqp] stale HIP error before %s (%s:%d): %s\n", #expr, __FILE__, __LINE__, hipGetErrorString(_s)); \
    }                                                                                    \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                  \
      return MI_OSQP_ERR_DEVICE;                                                         \
    }                                                                                    \
  } while (0)

// Every entry point that touches the device runs with the handle's device current and restores the caller's afterwards:
// a handle may be used from any host thread, whatever device that thread had selected.
struct DevGuard {
  int prev = -1; bool switched = false;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
  DevGuard(const DevGuard &) = delete;
  DevGuard &operator=(const DevGuard &) = delete;
};

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// MI_OSQP_DEBUG_TIMING: wall time of the C-ABI calls that sit in the GOMP drivers' loops, summed per entry point and
// printed when the process exits
struct CallTimer {
  struct Slot { const char *name; double s; long calls; };
  static Slot *slots() { static Slot t[16] = {}; return t; }
  static bool on() { static const bool v = getenv("MI_OSQP_DEBUG_TIMING") != nullptr; return v; }
  static void report() {
    for (Slot *t = slots(); t->name; t++) fprintf(stderr, "[mi_osqp] %-28s %6ld calls %9.3f ms\n", t->name, t->calls, 1e3 * t->s);
  }
  const char *name; double t0;
  explicit CallTimer(const char *n) : name(n), t0(on() ? now_s() : 0.0) {}
  ~CallTimer() {
    if (!on()) return;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    Slot *t = slots();
    static bool registered = false;
    if (!registered) { atexit(report); registered = true; }
    while (t->name && t->name != name && t < slots() + 14) t++;
    t->name = name; t->s += now_s() - t0; t->calls++;
  }
};

// cores this process may use: min(hardware threads, cgroup CPU quota); the GPU
// boxes expose 256 logical CPUs but grant a quota of ~16
static int host_threads() {
  static int cached = 0;
  if (cached) return cached;
  const char *e = getenv("MI_OSQP_HOST_THREADS");
  int t = (int)std::thread::hardware_concurrency();
  if (e) t = atoi(e);
  else {
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[64]; long long period = 0;
      if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
        t = std::min<long long>(t, std::max<long long>(1, (atoll(q) + period / 2) / period));
      fclose(f);
    }
    long long q1 = -1, p1 = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(f, "%lld", &q1) != 1) q1 = -1; fclose(f); }
    if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(f, "%lld", &p1) != 1) p1 = 0; fclose(f); }
    if (q1 > 0 && p1 > 0) t = std::min<long long>(t, std::max<long long>(1, (q1 + p1 / 2) / p1));
  }
  cached = std::max(1, std::min(t, 128));
  return cached;
}

template <class F>
static void parallel_for(int count, F &&fn) {
  int nt = std::min(host_threads(), count);
  if (nt <= 1) { for (int i = 0; i < count; i++) fn(i, 0); return; }
  std::atomic<int> next{0};
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++)
    th.emplace_back([&, t]() { for (int i; (i = next.fetch_add(1)) < count;) fn(i, t); });
  for (auto &x : th) x.join();
}

// Device memory of freed handles is kept for the next one (the GOMP drivers build a new solver per horizon segment:
// hipMalloc / hipFree of ~60 buffers cost ~11 ms per segment otherwise).  A block is reused for requests between half
// its size and its size; at most 8 GiB are kept, mi_osqp_release_device_cache() returns them to the runtime.
namespace devpool {
static std::mutex mu;
static std::multimap<std::pair<int, size_t>, void *> blocks;      // (device, capacity in bytes) -> pointer
static size_t kept = 0;
constexpr size_t kMaxKept = (size_t)8 << 30;
static void *take(int dev, size_t bytes, size_t &cap) {
  std::lock_guard<std::mutex> lk(mu);
  auto it = blocks.lower_bound({dev, bytes});
  if (it == blocks.end() || it->first.first != dev || it->first.second > 2 * bytes + 4096) return nullptr;
  void *p = it->second; cap = it->first.second; kept -= cap;
  blocks.erase(it);
  return p;
}
static bool give(int dev, void *p, size_t cap) {
  std::lock_guard<std::mutex> lk(mu);
  if (kept + cap > kMaxKept) return false;
  blocks.emplace(std::make_pair(dev, cap), p); kept += cap;
  return true;
}
static void release_all() {
  std::lock_guard<std::mutex> lk(mu);
  for (auto &b : blocks) (void)hipFree(b.second);
  blocks.clear(); kept = 0;
}
}  // namespace devpool

// The same for pinned host memory and for streams + events: hipHostMalloc costs ~0.5 ms per call and a handle needs four
// of them, a stream and five events - 2-3 ms of a 4 ms setup for the small QPs of a sequential GOMP run.
// (pipe_r / pipe_i / pipe_x / pipe_ev: the streams and the events of a pipelined refactorisation, created by the first handle
//  that needs them and handed on with the bundle; null until then)
namespace hostpool {
static std::mutex mu;
static std::multimap<size_t, void *> blocks;          // capacity in bytes -> pinned pointer
static size_t kept = 0;
constexpr size_t kMaxKept = (size_t)1 << 30;
static void *take(size_t bytes, size_t &cap) {
  std::lock_guard<std::mutex> lk(mu);
  auto it = blocks.lower_bound(bytes);
  if (it == blocks.end() || it->first > 4 * bytes + 65536) return nullptr;
  void *p = it->second; cap = it->first; kept -= cap;
  blocks.erase(it);
  return p;
}
static void give(void *p, size_t cap) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (kept + cap <= kMaxKept) { blocks.emplace(cap, p); kept += cap; return; }
  }
  (void)hipHostFree(p);
}
static void release_all() {
  std::lock_guard<std::mutex> lk(mu);
  for (auto &b : blocks) (void)hipHostFree(b.second);
  blocks.clear(); kept = 0;
}
// pinned allocation of at least `bytes` (rounded up to 4 KiB); *cap = what to hand back to give()
static hipError_t alloc(void **p, size_t bytes, size_t *cap) {
  bytes = (bytes + 4095) & ~(size_t)4095;
  if (void *q = take(bytes, *cap)) { *p = q; return hipSuccess; }
  *cap = bytes;
  return hipHostMalloc(p, bytes, hipHostMallocPortable);      // (a kept block may serve a handle on another device)
}
}  // namespace hostpool
namespace streampool {
constexpr int kPipeChunks = 8;                      // refactorisation chunks of a pipelined region, at most
constexpr int kPipeLanes = 3;                       // chunk lanes, at most: with the solve stream four streams, the hardware queues a process gets by default
constexpr int kPipeEvents = 3 + 3 * kPipeChunks + kPipeLanes + 1;    // fork, begin / end of the iterates, (begin, factor done, tail done) per chunk, end of every lane, end of the chain's stream
// lane_prio: the stream priority pipe_r / pipe_i / pipe_x were created with (a stream keeps it for life; MI_OSQP_REGION_PRIORITY
// = 1 asks for the least one) - a handle that wants another destroys them and creates its own (setup).  pipe_c, the
// stream of the run-ahead chain under MI_OSQP_REGION_PRIORITY = 2, is only ever created at the greatest priority.
struct Bundle { int dev; hipStream_t stream; hipEvent_t ev[5]; hipStream_t pipe_r, pipe_i, pipe_x; hipEvent_t pipe_ev[kPipeEvents]; int lane_prio; hipStream_t pipe_c; };
static void destroy(const Bundle &b) {
  for (hipEvent_t e : b.ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : b.pipe_ev) if (e) (void)hipEventDestroy(e);
  for (hipStream_t st : {b.stream, b.pipe_r, b.pipe_i, b.pipe_x, b.pipe_c}) if (st) (void)hipStreamDestroy(st);
}
static std::mutex mu;
static std::vector<Bundle> idle;
static bool take(int dev, Bundle &out) {
  std::lock_guard<std::mutex> lk(mu);
  for (size_t i = 0; i < idle.size(); i++)
    if (idle[i].dev == dev) { out = idle[i]; idle.erase(idle.begin() + i); return true; }
  return false;
}
static void give(const Bundle &b) {           // (the stream has been synchronised)
  {
    std::lock_guard<std::mutex> lk(mu);
    if (idle.size() < 64) { idle.push_back(b); return; }
  }
  destroy(b);
}
static void release_all() {
  std::lock_guard<std::mutex> lk(mu);
  for (Bundle &b : idle) destroy(b);
  idle.clear();
}
}  // namespace streampool

template <class T>
struct DevBuf {
  T *p = nullptr; size_t n = 0;
  size_t cap = 0;            // bytes of the underlying block
  int dev = 0;               // the device it lives on
  int alloc(size_t count) {
    free();
    n = count;
    if (!count) return 0;
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (void *q = devpool::take(dev, bytes, cap)) { p = (T *)q; return 0; }
    hipError_t e = hipMalloc((void **)&p, bytes);
    if (e != hipSuccess) {          // the kept blocks may be what is in the way
      devpool::release_all();
      e = hipMalloc((void **)&p, bytes);
    }
    if (e != hipSuccess) { p = nullptr; g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e); return MI_OSQP_ERR_ALLOC; }
    cap = bytes;
    return 0;
  }
  int zero(hipStream_t s) { if (n && hipMemsetAsync(p, 0, n * sizeof(T), s) != hipSuccess) return MI_OSQP_ERR_DEVICE; return 0; }
  int upload(const std::vector<T> &v) {
    int rc = alloc(v.size());
    if (rc) return rc;
    if (v.size() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return MI_OSQP_ERR_DEVICE;
    return 0;
  }
  void free() { if (p && !devpool::give(dev, p, cap)) (void)hipFree(p); p = nullptr; n = 0; cap = 0; }
  ~DevBuf() { free(); }
};

struct SchedBufs {
  DevBuf<uint32_t> step, idxw, lvl_pos, tail_bar;
  DevBuf<uint64_t> idxw64;
  DevBuf<int32_t> src;
  int upload(const Schedule &s) {
    int rc;
    if ((rc = step.upload(s.step)) || (rc = idxw.upload(s.idxw)) || (rc = idxw64.upload(s.idxw64)) || (rc = src.upload(s.src)) ||
        (rc = lvl_pos.upload(s.lvl_pos)) || (rc = tail_bar.upload(s.tail_bar))) return rc;
    return 0;
  }
  SchedDev view(const Schedule &s) const {
    SchedDev d; d.step = step.p; d.idxw = idxw.p; d.idxw64 = idxw64.p; d.lvl_pos = lvl_pos.p; d.tail_bar = tail_bar.p;
    d.n_phases = s.n_phases; d.nw = s.nw; d.n_levels = s.n_levels;
    d.n_steps = s.n_steps; d.n_slots = s.n_slots;
    return d;
  }
};

struct mi_osqp_batch {
  Settings st;
  bool rho_interval_auto = false;             // setup derived st.adaptive_rho_interval from 0 (a settings update may pass 0 again)
  Tuning tune;                                // the MI_OSQP_* switches, read once at setup (tuning_from_env)
  std::shared_ptr<const Analysis> anp;        // pattern analysis: shared between the handles of one pattern (analysis cache below)
  int B = 0, BT = 1, ntiles = 0, threads = 512, device = 0, n_cus = 256;
  size_t lds = 0;
  size_t lds_iter = 0;                        // LDS of the iterate / advance launches: lds + the resident state where it fits (rs_off != 0)
  int rs_off = 0;                             // KernelArgs::rs_off
  size_t lds_factor = 0;                      // LDS part of the resident head of S^-1, behind the resident state (iterate launches only)
  int rf_off = 0, rf_steps = 0;               // KernelArgs::rf_off; steps per wave the head keeps (registers + LDS; of the long form unless the deep ring is forced), 0 = streamed
  int ix = 0;                                 // KernelArgs::ix: the iterate launches keep their index words in registers (index_words_fit, MI_OSQP_INDEX_LOADS)
  int64_t rf_launches[3] = {0, 0, 0};         // iterate launches since setup by form (RF_FORM_*; chunk iterates count one each)
  std::vector<QPNumeric> qp;
  bool host_bounds_stale = false;
  hipStream_t stream = nullptr;
  SchedBufs fwd, bwd, chk;
  DevBuf<uint32_t> pinv, xloc;
  DevBuf<double> fwd_val, bwd_val, chk_val, dinv, x, z, y, q, l, u, rho_vec, rho_inv, Dsc, Dsc_inv, Esc, Esc_inv;
  DevBuf<double> dx, dy, out1, out2, dscal, x_out, y_out, xs_global;
  DevBuf<double> cert_out;                    // infeasibility certificates, [B][max(n, m, 1)] (KernelArgs::cert_out)
  bool global_xs = false;
  int mw_groups = 0, mw_threads = 0;    // > 0: dataflow form of the solves (Analysis::df): mw_groups workgroups of mw_threads threads share the ONE QP of the handle
  DevBuf<uint32_t> mw_bar;              // their grid barrier: arrival count, generation, error word
  DevBuf<unsigned char> rflag;
  DevBuf<double> mw_scratch;            // partial norms / sums of the grid-wide check_kernel
  DevBuf<double> fwd_val0, bwd_val0, dinv0, rho_vec0, rho_inv0, dscal0;   // setup snapshot (reset)
  DevBuf<int> use_work;                       // per slot: the current factor is the working copy (KernelArgs::use_work)
  DevBuf<int> iscal, flag, npos;
  // device refactorisation (BlockFactor tables + scratch)
  DevBuf<uint32_t> bf_blk, bf_lvl, bf_utask, bf_tri, bf_dtask, bf_ttask, bf_asm_dst, bf_asm_src, bf_ubig;
  DevBuf<int32_t> fwd_srcblk, bwd_srcblk;
  DevBuf<double> pa_val, Lblk, Dl, dinv_scratch;
  // dense tail (host_core.hpp DenseTail): task tables, the per-QP stream of S^-1 (+ setup snapshot), dense scratch
  DevBuf<uint32_t> dt_task, dt_wave_task, dt_wave_step, dt_tail_bar;
  DevBuf<uint32_t> dt_lt_pos, dt_ltcol_col, dt_tile_tab, dt_wave_tiles, dt_diag_tile, dt_task_step;     // tail_kernel tables
  DevBuf<uint64_t> dt_asm_q64;
  DevBuf<int32_t> dt_src_tile;
  int dt_nh = 0; uint32_t dt_cs_doubles = 0; size_t dt_lds = 0, dt_lds_asm = 0;
  DevBuf<int32_t> dt_src;
  DevBuf<double> dt_val, dt_val0, dt_Sd;
  DevBuf<uint32_t> sp_ptr, sp_ent;      // fused SpMV op (spmv_fused_kernel); empty when not eligible
  DevBuf<uint32_t> sp_ell, sp_rowid;    // its prefetching form (rows sorted by length, <= 4 passes of 512 rows, <= 24 entries per row)
  int sp_npass = 0;
  uint32_t sp_ell_off[4] = {0, 0, 0, 0}, sp_ell_k[4] = {0, 0, 0, 0};
  bool host_rho_stale = false;
  bool host_scaling_stale = false;      // the device has re-equilibrated (ruiz_kernel): P, A, q, D, E, c of the host mirrors lag behind
  DevBuf<int32_t> rz_prow, rz_pcol, rz_arow, rz_acol;      // per entry of triu(P) / A: row, column (row E2 on the device)
  bool clear_rho_updates = true;          // the next solve starts counting rho updates from 0 (setup / update_* / reset happened)
  int *h_npos = nullptr;
  DevBuf<double> stage; DevBuf<int> ids, work;
  int *h_iscal = nullptr;     // pinned (hostpool; *_cap = capacity to hand back)
  double *h_dscal = nullptr;  // pinned
  size_t h_iscal_cap = 0, h_dscal_cap = 0, h_npos_cap = 0, pin_cap = 0;
  double *pin = nullptr;      // pinned staging of the host update paths (a pageable hipMemcpy runs at ~1 GB/s here, and unevenly)
  size_t pin_n = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evf0 = nullptr, evf1 = nullptr, evf2 = nullptr;
  // pipelined refactorisation (solve_impl): stream R of the refactorisation chunks, stream I of the chunk iterates, their events;
  // with chunk lanes the three are lanes 0, 1, 2 (pipe_x is only ever the third lane)
  hipStream_t pipe_r = nullptr, pipe_i = nullptr, pipe_x = nullptr;
  hipEvent_t pipe_ev[streampool::kPipeEvents] = {};
  // MI_OSQP_REGION_PRIORITY (setup): the form in effect (0 where the device reports one stream priority only), the priority
  // the lanes are created with, the chain's stream of form 2 (created with the first region that runs ahead)
  int prio_form = 0, lane_prio = 0, chain_prio = 0;
  bool prio_inert = false;
  hipStream_t pipe_c = nullptr;
  int64_t region_priority = 0, region_lane_checks = 0, region_chunks = 0;      // mi_osqp_stats region_*: the last region
  DevBuf<int> tile_list;                      // the active tiles chunk after chunk (KernelArgs::tiles)
  int64_t pipelined_refactors = 0;            // rho-update points of this handle that took the pipelined form
  int64_t refactor_lanes = 0;                 // the most chunk lanes one of them ran on (1 = the two-stream form)
  // run-ahead (solve_impl): five lists of ntiles entries - the tiles of the main loop's launches, the group, the group's
  // flagged slots, the device-built work list of the chain, the marks of the slots the chain failed - and the residuals of
  // the running QPs (KernelArgs::res)
  DevBuf<int> ra_list;
  DevBuf<double> ra_res;
  double *h_res = nullptr; int *h_mark = nullptr;      // pinned images of ra_res and of the marks
  size_t h_res_cap = 0, h_mark_cap = 0;
  int64_t ra_regions = 0, ra_tiles = 0, ra_left = 0, ra_missed = 0;      // mi_osqp_stats runahead_*
  double factor_ms_sum = 0.0, dense_ms_sum = 0.0;
  int64_t refactor_launches = 0, refactor_qps = 0, peak_qps = 0;
  double peak_factor_ms = 0.0, peak_tail_ms = 0.0;
  mi_osqp_stats stats{};
  // last-solve accounting
  int64_t last_total_iters = 0, last_launches = 0, last_refactors = 0;
  double last_device_s = 0.0, last_refactor_s = 0.0, kernel_ms_sum = 0.0;
  int64_t kernel_launches = 0, kernel_qp_iters = 0;
  bool solved_once = false;             // the status words of iscal are valid: a blocking solve has finished, or the continuous mode was entered
  // per-QP failure isolation: QPs whose KKT factor lost its inertia (at setup, in an update or in a rho update).  They
  // report kNonConvex with a NaN solution on every solve until a later refactorisation of theirs succeeds; the rest
  // of the batch is unaffected ([REF] src/osqp-wrapper.h:51-54: solve() never throws, one exit code per solver).
  std::vector<char> failed;
  DevBuf<int> fail_list;
  // raw triu(P) and q as setup received them ([QP][nnzP], [QP][n]): what mi_osqp_batch_reinit_some equilibrates from
  DevBuf<double> rawP, rawq;
  // solution polishing (section "polish"): the polish factor's streams / dinv / dense-tail stream, the refinement iterate,
  // the active set and the per-QP state - allocated at the first polish of the handle; the ADMM factor never reads them
  DevBuf<double> pol_fwd, pol_bwd, pol_dinv, pol_dt, pol_sol;
  DevBuf<signed char> pol_act;
  DevBuf<int> pol_stat;
  std::vector<int> pol_status;          // per QP: status_polish of the last solve (empty: nothing polished yet)
  int64_t pol_count = 0, pol_accepted = 0;
  double pol_seconds = 0.0;
  hipEvent_t evp0 = nullptr, evp1 = nullptr;
  DevBuf<int> adj_stat;                 // adjoint derivative (section "adjoint"): its own per-QP marks / results (pol_stat belongs to the polish)
  // ---- continuous batching (the per-QP entry points + advance / poll; section "continuous" below)
  struct Cont {
    bool on = false;
    int L = 25;                              // iterations per segment (gcd of the check / rho / max_iter periods)
    unsigned launch_seq = 0;                 // sequence number of the last advance launch (the stop word's currency)
    DevBuf<unsigned> stop;                   // device word: launch in which a QP last finished (advance_kernel)
    int64_t adv_seq = 0, polled_seq = 0;     // segments enqueued / segments whose flags the host has read
    std::vector<char> running, clear_rho;    // per QP: a solve is in flight; its next solve counts rho updates from 0
    std::vector<mi_osqp_info> info;          // per QP: result of its last finished solve
    int n_running = 0;
    // flag copies of the last two advances (pinned): iscal / dscal images + the event behind them
    int *h_is[2] = {nullptr, nullptr}; double *h_ds[2] = {nullptr, nullptr}; size_t h_is_cap[2] = {0, 0}, h_ds_cap[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr}; int64_t seq_of[2] = {0, 0};
    // solutions of finished QPs land in pinned host memory straight from check_kernel ([B][n], [B][m])
    double *xh = nullptr, *yh = nullptr; size_t xh_cap = 0, yh_cap = 0;
    double *ch = nullptr; size_t ch_cap = 0;      // and the infeasibility certificates ([B][max(n, m, 1)], KernelArgs::cert_out)
    // per QP: the status under which get_*_inf_cert_some read its row of ch - what poll() reported for its last finished solve,
    // 0 (no certificate) from the begin of its next solve or a reinit on; cont.info keeps the last report meanwhile
    std::vector<int> cert_status;
    // staging ring of the per-QP calls: regions are handed out once per call and recycled when the ring wraps (after a
    // synchronisation), so a call never waits for an earlier call's copy
    char *ring_h = nullptr; size_t ring_cap = 0, ring_h_cap = 0, ring_head = 0;
    int64_t ring_wraps = 0;                  // times the ring has wrapped (mi_osqp_batch_ring_wraps)
    DevBuf<char> ring_d;
    DevBuf<int> work;                        // device-built refactorisation work list of an advance
    // The per-QP calls (new data, equilibration, refactorisation, warm start, begin) and the refactorisations after rho
    // updates are enqueued on the handle's stream behind the advance launches.  A begun solve carries a pending mark that the
    // next advance launch to see it takes up (IS_PENDING), a QP whose rho changed pauses until its refactorisation has run,
    // and the host tells a finished solve from the slot's previous one by its epoch (IS_EPOCH).
    hipEvent_t ev_adv = nullptr;             // behind the last advance launch (the refactorisation kernels wait for it)
    std::vector<int> epoch;                  // per QP: solves begun so far (what IS_EPOCH reads once the begin has run)
    DevBuf<double> rz_scratch;               // equilibration scratch of the per-QP calls (not the check kernels')
    double *keepA = nullptr, *keepl = nullptr, *keepu = nullptr;   // a mi_gomp_scene's QP-major copy of the raw rows: reinit / update keep it current
    DevBuf<unsigned> counter;                // tiles that have left the advance launch in flight
    unsigned *h_done = nullptr; size_t h_done_cap = 0;      // pinned: [0] sequence number of the last advance launch that is over, [1] tiles that iterated in it
    // polishing on demand (mi_osqp_batch_polish_some).  Per QP: polishable = poll() reported its solve kOptimal and nothing has
    // touched it since; polishing = a polish is enqueued and not reported yet (the QP counts as running); pol_status = the
    // status_polish of its last solve.  h_pstat: pinned [slot] image polish_publish_kernel writes the results into.
    std::vector<char> polishable, polishing;
    std::vector<int> pol_status;
    int *h_pstat = nullptr; size_t h_pstat_cap = 0;
  } cont;
  ~mi_osqp_batch() {
    DevGuard guard(device);
    if (stream) (void)hipStreamSynchronize(stream);      // (the buffers go back to their pools right after: DevBuf remembers its device)
    for (int k = 0; k < 2; k++) { hostpool::give(cont.h_is[k], cont.h_is_cap[k]); hostpool::give(cont.h_ds[k], cont.h_ds_cap[k]); if (cont.ev[k]) (void)hipEventDestroy(cont.ev[k]); }
    hostpool::give(cont.xh, cont.xh_cap); hostpool::give(cont.yh, cont.yh_cap); hostpool::give(cont.ch, cont.ch_cap); hostpool::give(cont.ring_h, cont.ring_h_cap);
    if (cont.ev_adv) (void)hipEventDestroy(cont.ev_adv);
    if (evp0) (void)hipEventDestroy(evp0);
    if (evp1) (void)hipEventDestroy(evp1);
    hostpool::give(cont.h_done, cont.h_done_cap); hostpool::give(cont.h_pstat, cont.h_pstat_cap);
    hostpool::give(h_iscal, h_iscal_cap); hostpool::give(h_dscal, h_dscal_cap); hostpool::give(pin, pin_cap); hostpool::give(h_npos, h_npos_cap);
    hostpool::give(h_res, h_res_cap); hostpool::give(h_mark, h_mark_cap);
    if (pipe_r) (void)hipStreamSynchronize(pipe_r);
    if (pipe_i) (void)hipStreamSynchronize(pipe_i);
    if (pipe_x) (void)hipStreamSynchronize(pipe_x);
    if (pipe_c) (void)hipStreamSynchronize(pipe_c);
    streampool::Bundle sb{device, stream, {ev0, ev1, evf0, evf1, evf2}, pipe_r, pipe_i, pipe_x, {}, lane_prio, pipe_c};
    for (int k = 0; k < streampool::kPipeEvents; k++) sb.pipe_ev[k] = pipe_ev[k];
    if (stream && ev0 && ev1 && evf0 && evf1 && evf2) streampool::give(sb);
    else streampool::destroy(sb);
  }
};

struct mi_osqp_solver { mi_osqp_batch *b = nullptr; };

// ------------------------------------------------------------------ helpers

static Settings to_settings(const mi_osqp_settings *s) {
  Settings t;
  if (!s) return t;
  t.rho = s->rho; t.sigma = s->sigma; t.scaling = s->scaling; t.adaptive_rho = s->adaptive_rho;
  t.adaptive_rho_interval = s->adaptive_rho_interval; t.adaptive_rho_tolerance = s->adaptive_rho_tolerance;
  t.max_iter = s->max_iter; t.eps_abs = s->eps_abs; t.eps_rel = s->eps_rel; t.eps_prim_inf = s->eps_prim_inf;
  t.eps_dual_inf = s->eps_dual_inf; t.alpha = s->alpha; t.scaled_termination = s->scaled_termination;
  t.check_termination = s->check_termination; t.warm_start = s->warm_start; t.verbose = s->verbose;
  t.polish = s->polish; t.polish_refine_iter = s->polish_refine_iter; t.delta = s->delta;
  return t;
}

// the deal of the dense-tail product over the waves of a tile (host_core.cpp build_dense_tail), for stats()
static void dense_tail_deal_stats(const DenseTail &dt, mi_osqp_stats &s) {
  s.dense_tail_tasks = s.dense_tail_waves_used = s.dense_tail_wave_tasks_max = 0;
  if (!dt.k) return;
  s.dense_tail_tasks = (int64_t)dt.task.size() / 4;
  for (int w = 0; w < dt.nw; w++) {
    const int64_t c = (int64_t)dt.wave_task[w + 1] - (int64_t)dt.wave_task[w];
    s.dense_tail_waves_used += c > 0; s.dense_tail_wave_tasks_max = std::max(s.dense_tail_wave_tasks_max, c);
  }
}

static size_t lds_bytes(int N, int BT, int threads) {
  int nw = threads / 64;
  return ((size_t)N * BT + (size_t)nw * 14 * BT + 14 * BT) * sizeof(double);
}

static KernelArgs make_args(mi_osqp_batch *h) {
  KernelArgs a{};
  a.n = (*h->anp).n; a.m = (*h->anp).m; a.N = (*h->anp).N; a.B = h->B;
  a.fwd = h->fwd.view((*h->anp).fwd); a.bwd = h->bwd.view((*h->anp).bwd); a.chk = h->chk.view((*h->anp).chk);
  a.pinv = h->pinv.p; a.xloc = h->xloc.p;
  a.fwd_val = h->fwd_val.p; a.bwd_val = h->bwd_val.p; a.chk_val = h->chk_val.p; a.dinv = h->dinv.p;
  a.fwd_val0 = h->fwd_val0.p; a.bwd_val0 = h->bwd_val0.p; a.dt_val0 = h->dt_val0.p;
  a.use_work = (h->fwd_val0.p && h->bwd_val0.p && (!(*h->anp).dt.k || h->dt_val0.p)) ? h->use_work.p : nullptr;     // (before the first snapshot: working copy only)
  a.x = h->x.p; a.z = h->z.p; a.y = h->y.p; a.q = h->q.p; a.l = h->l.p; a.u = h->u.p;
  a.rho_vec = h->rho_vec.p; a.rho_inv = h->rho_inv.p; a.Dsc = h->Dsc.p; a.Dsc_inv = h->Dsc_inv.p;
  a.Esc = h->Esc.p; a.Esc_inv = h->Esc_inv.p; a.dx = h->dx.p; a.dy = h->dy.p; a.out1 = h->out1.p; a.out2 = h->out2.p;
  a.dscal = h->dscal.p; a.iscal = h->iscal.p;
  a.x_out = h->x_out.p; a.y_out = h->y_out.p;
  a.cert_out = h->cert_out.p; a.cert_stride = (int)std::max<int64_t>(std::max<int64_t>(a.n, a.m), 1);
  a.xs_global = h->global_xs ? h->xs_global.p : nullptr; a.xs_len = (*h->anp).xs_total; a.wide = (*h->anp).wide ? 1 : 0;
  a.rs_off = h->rs_off; a.rf_off = h->rf_off; a.ix = h->ix;
  a.rf_form = iterate_form(h->ntiles, h->rf_off != 0, h->tune);      // (solve_impl sets it per launch from the tiles still iterating)
  a.mw_groups = h->mw_groups; a.mw_bar = h->mw_bar.p; a.mw_scratch = h->mw_scratch.p;
  a.df = (*h->anp).df ? 1 : 0; a.df_shadow = (unsigned)(*h->anp).Next; a.rflag = h->rflag.p;
  {
    const DenseTail &dt = (*h->anp).dt;
    a.dt.s = dt.s; a.dt.k = dt.k; a.dt.n_phases = dt.n_phases; a.dt.n_steps = dt.n_steps;
    a.dt.task = h->dt_task.p; a.dt.wave_task = h->dt_wave_task.p; a.dt.wave_step = h->dt_wave_step.p; a.dt.tail_bar = h->dt_tail_bar.p;
    a.dt_val = h->dt_val.p;
  }
  const Settings &s = h->st;
  a.sigma = s.sigma; a.alpha = s.alpha; a.eps_abs = s.eps_abs; a.eps_rel = s.eps_rel;
  a.eps_prim_inf = s.eps_prim_inf; a.eps_dual_inf = s.eps_dual_inf; a.rho_tolerance = s.adaptive_rho_tolerance;
  a.check_termination = (int)s.check_termination; a.rho_interval = (int)s.adaptive_rho_interval;
  a.max_iter = (int)s.max_iter; a.scaled_termination = (int)s.scaled_termination; a.scaling = s.scaling ? 1 : 0;
  a.adaptive_rho = (int)s.adaptive_rho; a.iter_begin = 0; a.iter_end = 0; a.info_at_end = 1;
  return a;
}

static FactorArgs make_factor_args(mi_osqp_batch *h, int force_all) {
  FactorArgs a{};
  const Analysis &an = (*h->anp);
  a.n = an.n; a.m = an.m; a.N = an.N; a.B = h->B; a.nnzP = an.Pp[an.n]; a.nnzK = an.nnzK();
  a.pa_len = an.Pp[an.n] + an.Ap[an.n]; a.n_levels = an.bf.n_levels; a.force_all = force_all;
  a.storage = an.bf.storage; a.fwd = h->fwd.view(an.fwd); a.bwd = h->bwd.view(an.bwd);
  a.blk = h->bf_blk.p; a.lvl = h->bf_lvl.p; a.utask = h->bf_utask.p; a.tri4 = h->bf_tri.p; a.dtask = h->bf_dtask.p; a.ubig = h->bf_ubig.p;
  a.ttask = h->bf_ttask.p; a.asm_dst = h->bf_asm_dst.p; a.asm_src = h->bf_asm_src.p;
  a.fwd_srcblk = h->fwd_srcblk.p; a.bwd_srcblk = h->bwd_srcblk.p;
  a.pa_val = h->pa_val.p; a.l = h->l.p; a.u = h->u.p; a.dscal = h->dscal.p;
  a.rho_vec = h->rho_vec.p; a.rho_inv = h->rho_inv.p; a.Lblk = h->Lblk.p; a.Dl = h->Dl.p; a.dinv_scratch = h->dinv_scratch.p;
  a.fwd_val = h->fwd_val.p; a.bwd_val = h->bwd_val.p; a.dinv = h->dinv.p; a.iscal = h->iscal.p; a.npos = h->npos.p; a.use_work = h->use_work.p;
  a.sigma = h->st.sigma; a.home_bt = h->BT; a.dt_k = an.dt.k;
  a.mw_groups = 0; a.mw_bar = h->mw_bar.p;      // (device_refactor_slots decides how many workgroups share a QP)
#ifdef MI_OSQP_DEBUG_BUILD
  { const char *e = getenv("MI_OSQP_FACTOR_SKIP"); a.debug_skip = e ? atoi(e) : 0; }      // timing experiments, diagnostic build only
#endif
  return a;
}

static int ensure_stage(mi_osqp_batch *h, size_t doubles, size_t ints) {
  int rc;
  if (h->stage.n < doubles && (rc = h->stage.alloc(doubles))) return rc;
  if (h->ids.n < ints && (rc = h->ids.alloc(ints))) return rc;
  return 0;
}

static int ensure_pin(mi_osqp_batch *h, size_t doubles) {
  if (h->pin_n >= doubles) return 0;
  if (h->pin) { hostpool::give(h->pin, h->pin_cap); h->pin = nullptr; h->pin_n = 0; }
  HIPCHK(hostpool::alloc((void **)&h->pin, doubles * sizeof(double), &h->pin_cap));
  h->pin_n = h->pin_cap / sizeof(double);
  return 0;
}
// memcpy on the host threads (user arrays of several MB per call in the GOMP drivers' loops)
static void par_copy(double *dst, const double *src, size_t n) {
  const size_t chunk = (size_t)1 << 17;       // 1 MiB
  const int parts = (int)((n + chunk - 1) / chunk);
  if (parts <= 2) { memcpy(dst, src, n * sizeof(double)); return; }
  parallel_for(parts, [&](int i, int) { const size_t b = (size_t)i * chunk; memcpy(dst + b, src + b, std::min(chunk, n - b) * sizeof(double)); });
}

// upload QP-major host rows [nq][len] into a tile-interleaved device array
static int upload_rows(mi_osqp_batch *h, const std::vector<double> &rows, const std::vector<int> *ids, int nq,
                       int len, double *dst) {
  if (!nq || !len) return 0;
  int rc = ensure_stage(h, rows.size(), ids ? ids->size() : 0);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(h->stage.p, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (ids) HIPCHK(hipMemcpyAsync(h->ids.p, ids->data(), ids->size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(launch_interleave(h->stage.p, dst, ids ? h->ids.p : nullptr, nq, len, h->BT, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

template <class G>
static std::vector<double> gather_rows(const std::vector<int> &ids, int len, G &&get) {
  std::vector<double> rows((size_t)ids.size() * len);
  for (size_t j = 0; j < ids.size(); j++) { const std::vector<double> &v = get(ids[j]); std::copy(v.begin(), v.begin() + len, rows.begin() + j * len); }
  return rows;
}

static int upload_rho(mi_osqp_batch *h, const std::vector<int> &ids) {
  int m = (*h->anp).m, nq = (int)ids.size(), rc;
  if (!nq || !m) return 0;
  std::vector<double> r1 = gather_rows(ids, m, [&](int q) -> const std::vector<double> & { return h->qp[q].rho_vec; });
  if ((rc = upload_rows(h, r1, &ids, nq, m, h->rho_vec.p))) return rc;
  std::vector<double> r2 = gather_rows(ids, m, [&](int q) -> const std::vector<double> & { return h->qp[q].rho_inv; });
  return upload_rows(h, r2, &ids, nq, m, h->rho_inv.p);
}

// scaled problem data, scalings, scalars of the listed QPs
static int upload_problem(mi_osqp_batch *h, const std::vector<int> &ids, bool with_matrices) {
  const Analysis &an = (*h->anp);
  int n = an.n, m = an.m, nq = (int)ids.size(), rc;
  if (!nq) return 0;
  auto up = [&](int len, double *dst, auto get) -> int {
    std::vector<double> rows = gather_rows(ids, len, get);
    return upload_rows(h, rows, &ids, nq, len, dst);
  };
  if (with_matrices) {
    int nnzP = an.Pp[n], nnzA = an.Ap[n];
    std::vector<double> pa((size_t)nq * (nnzP + nnzA));
    for (int j = 0; j < nq; j++) {
      const QPNumeric &q = h->qp[ids[j]];
      std::copy(q.Pv.begin(), q.Pv.end(), pa.begin() + (size_t)j * (nnzP + nnzA));
      std::copy(q.Av.begin(), q.Av.end(), pa.begin() + (size_t)j * (nnzP + nnzA) + nnzP);
    }
    if ((rc = ensure_stage(h, std::max<size_t>(pa.size(), 1), ids.size()))) return rc;
    HIPCHK(hipMemcpyAsync(h->ids.p, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (!pa.empty()) {
      HIPCHK(hipMemcpyAsync(h->stage.p, pa.data(), pa.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHK(launch_scatter(h->stage.p, h->chk_val.p, h->chk.src.p, h->ids.p, nq, nnzP + nnzA, h->chk.view(an.chk), h->BT, h->stream));
      HIPCHK(launch_interleave(h->stage.p, h->pa_val.p, h->ids.p, nq, nnzP + nnzA, h->BT, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    if ((rc = up(n, h->q.p, [&](int q) -> const std::vector<double> & { return h->qp[q].q; }))) return rc;
    if ((rc = up(n, h->Dsc.p, [&](int q) -> const std::vector<double> & { return h->qp[q].D; }))) return rc;
    if ((rc = up(n, h->Dsc_inv.p, [&](int q) -> const std::vector<double> & { return h->qp[q].Dinv; }))) return rc;
    if ((rc = up(m, h->Esc.p, [&](int q) -> const std::vector<double> & { return h->qp[q].E; }))) return rc;
    if ((rc = up(m, h->Esc_inv.p, [&](int q) -> const std::vector<double> & { return h->qp[q].Einv; }))) return rc;
  }
  if ((rc = up(m, h->l.p, [&](int q) -> const std::vector<double> & { return h->qp[q].l; }))) return rc;
  if ((rc = up(m, h->u.p, [&](int q) -> const std::vector<double> & { return h->qp[q].u; }))) return rc;
  return 0;
}

// write c, cinv, rho of the listed QPs into dscal (read-modify-write via host mirror)
static int sync_scalars_to_device(mi_osqp_batch *h, const std::vector<int> &ids, bool with_c) {
  size_t cnt = (size_t)h->ntiles * DS_COUNT * h->BT;
  HIPCHK(hipMemcpy(h->h_dscal, h->dscal.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
  for (int q : ids) {
    double *t = h->h_dscal + (size_t)(q / h->BT) * DS_COUNT * h->BT;
    int b = q % h->BT;
    if (with_c) { t[DS_C * h->BT + b] = h->qp[q].c; t[DS_CINV * h->BT + b] = h->qp[q].cinv; }
    t[DS_RHO * h->BT + b] = h->qp[q].rho;
    t[DS_RHO_EST * h->BT + b] = h->qp[q].rho;
  }
  HIPCHK(hipMemcpy(h->dscal.p, h->h_dscal, cnt * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

static int snapshot(mi_osqp_batch *h) {
  auto cp = [&](DevBuf<double> &dst, DevBuf<double> &src) -> int {
    if (dst.n != src.n) { int rc = dst.alloc(src.n); if (rc) return rc; }
    if (src.n) HIPCHK(hipMemcpyAsync(dst.p, src.p, src.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
  };
  // the factor streams: only the QPs whose current factor IS the working copy (the others' snapshot is current, and their
  // working copy may be a leftover of an earlier solve: a reset clears flags, it does not copy)
  const Analysis &an = (*h->anp);
  const int nslots = h->ntiles * h->BT;
  auto cps = [&](DevBuf<double> &dst, DevBuf<double> &src, size_t per) -> int {
    const bool fresh = dst.n != src.n;
    if (fresh) { int rc = dst.alloc(src.n); if (rc) return rc; }
    if (src.n) HIPCHK(launch_copy_flagged_streams(dst.p, src.p, fresh ? nullptr : h->use_work.p, 1, nslots, per, h->stream));
    return 0;
  };
  int rc;
  if ((rc = cps(h->fwd_val0, h->fwd_val, (size_t)an.fwd.phys_steps() * 64)) || (rc = cps(h->bwd_val0, h->bwd_val, (size_t)an.bwd.phys_steps() * 64)) ||
      (an.dt.k && (rc = cps(h->dt_val0, h->dt_val, (size_t)an.dt.n_steps * 64))) ||
      (rc = cp(h->dinv0, h->dinv)) || (rc = cp(h->rho_vec0, h->rho_vec)) || (rc = cp(h->rho_inv0, h->rho_inv)) || (rc = cp(h->dscal0, h->dscal))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// download scaled l,u from the device into the host mirrors (after device-side bound updates)
static int sync_bounds_to_host(mi_osqp_batch *h) {
  if (!h->host_bounds_stale) return 0;
  int m = (*h->anp).m, B = h->B, rc;
  if ((rc = ensure_stage(h, (size_t)B * m + 1, 0))) return rc;
  std::vector<double> tmp((size_t)B * m);
  for (int which = 0; which < 2; which++) {
    HIPCHK(launch_deinterleave(which ? h->u.p : h->l.p, h->stage.p, B, m, h->BT, h->stream));
    HIPCHK(hipMemcpyAsync(tmp.data(), h->stage.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int q = 0; q < B; q++) {
      std::vector<double> &dst = which ? h->qp[q].u : h->qp[q].l;
      std::copy(tmp.begin() + (size_t)q * m, tmp.begin() + (size_t)(q + 1) * m, dst.begin());
    }
  }
  h->host_bounds_stale = false;
  return 0;
}

// after device-side rho updates the host mirrors (rho, rho_vec) lag behind
static int sync_rho_to_host(mi_osqp_batch *h) {
  if (!h->host_rho_stale) return 0;
  int rc = sync_bounds_to_host(h);
  if (rc) return rc;
  size_t dcnt = (size_t)h->ntiles * DS_COUNT * h->BT;
  HIPCHK(hipMemcpy(h->h_dscal, h->dscal.p, dcnt * sizeof(double), hipMemcpyDeviceToHost));
  for (int q = 0; q < h->B; q++) {
    double r = h->h_dscal[(size_t)(q / h->BT) * DS_COUNT * h->BT + DS_RHO * h->BT + q % h->BT];
    if (r != h->qp[q].rho) apply_rho((*h->anp), h->qp[q], r);
  }
  h->host_rho_stale = false;
  return 0;
}

static int reset_solve_state(mi_osqp_batch *h, bool cold) {
  int rc;
  // statuses: UNSOLVED, not done (padding lanes of the last tile stay done)
  // (the count of rho updates survives a plain re-solve, as upstream's info->rho_updates does: only setup and the
  //  update_* calls reset it)
  size_t icnt = (size_t)h->ntiles * IS_COUNT * h->BT;
  for (int t = 0; t < h->ntiles; t++)
    for (int b = 0; b < h->BT; b++) {
      int *p = h->h_iscal + (size_t)t * IS_COUNT * h->BT;
      const int keep = h->clear_rho_updates ? 0 : p[IS_RHO_UPDATES * h->BT + b];
      for (int k = 0; k < IS_COUNT; k++) p[k * h->BT + b] = 0;
      p[IS_STATUS * h->BT + b] = -10;
      p[IS_DONE * h->BT + b] = (t * h->BT + b >= h->B) ? 1 : 0;
      p[IS_RHO_UPDATES * h->BT + b] = keep;
    }
  h->clear_rho_updates = false;
  HIPCHK(hipMemcpyAsync(h->iscal.p, h->h_iscal, icnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (cold) { if ((rc = h->x.zero(h->stream)) || (rc = h->z.zero(h->stream)) || (rc = h->y.zero(h->stream))) return rc; }
  return 0;
}

// ------------------------------------------------------------------- setup

// Pattern analysis (ordering, symbolic factor, step streams, block-factor and dense-tail tables) depends only on the
// sparsity pattern and the launch shape.  The GOMP drivers build one solver per horizon segment and the same ten
// patterns come back on every run(): the last analyses are kept (process-wide, keyed by a hash of the pattern, verified
// by a full comparison) and shared read-only between handles.  MI_OSQP_ANALYSIS_CACHE=0 switches the cache off.
namespace ancache {
struct Entry {
  uint64_t hash; int64_t n, m; int nw, bt, max_extra, dt_max, tri_waves, n_tiles; AnalysisTuning tune;
  std::vector<int64_t> Pp, Pi, Ap, Ai;
  std::shared_ptr<const Analysis> an;           // null while a thread is still computing it (mi_osqp_prefetch_analysis): others wait
};
static std::mutex mu;
static std::condition_variable cv;
static std::vector<Entry> entries;            // most recently used last
constexpr size_t kMaxEntries = 24;
static uint64_t fnv(uint64_t h, const void *p, size_t bytes) {
  const unsigned char *c = (const unsigned char *)p;
  for (size_t i = 0; i < bytes; i++) { h ^= c[i]; h *= 1099511628211ull; }
  return h;
}
}  // namespace ancache

static int cached_analysis(int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi, const int64_t *Ap, const int64_t *Ai, const Tuning &tune,
                           int nw, int bt, int max_extra, int dt_max, int tri_waves, int n_tiles, std::shared_ptr<const Analysis> &out) {
  n_tiles = n_tiles <= 1 ? 1 : (n_tiles <= 32 ? 32 : (n_tiles <= 128 ? 128 : (n_tiles <= 256 ? 256 : 512)));      // (buckets: the analysis is shared between handles)
  const bool use = tune.analysis_cache && n > 0 && m >= 0 && Pp && Ap && Pp[0] == 0 && Ap[0] == 0 && Pp[n] >= 0 && Ap[n] >= 0 &&
                   Pp[n] < ((int64_t)1 << 30) && Ap[n] < ((int64_t)1 << 30);
  uint64_t hsh = 1469598103934665603ull;
  auto same = [&](const ancache::Entry &e) {
    if (e.hash != hsh || e.n != n || e.m != m || e.nw != nw || e.bt != bt || e.max_extra != max_extra || e.dt_max != dt_max || e.tri_waves != tri_waves || e.n_tiles != n_tiles ||
        !(e.tune == tune.analysis)) return false;
    return (int64_t)e.Pi.size() == Pp[n] && (int64_t)e.Ai.size() == Ap[n] && !memcmp(e.Pp.data(), Pp, (size_t)(n + 1) * 8) &&
           !memcmp(e.Pi.data(), Pi, (size_t)Pp[n] * 8) && !memcmp(e.Ap.data(), Ap, (size_t)(n + 1) * 8) && !memcmp(e.Ai.data(), Ai, (size_t)Ap[n] * 8);
  };
  if (use) {
    hsh = ancache::fnv(hsh, Pp, (size_t)(n + 1) * 8); hsh = ancache::fnv(hsh, Pi, (size_t)Pp[n] * 8);
    hsh = ancache::fnv(hsh, Ap, (size_t)(n + 1) * 8); hsh = ancache::fnv(hsh, Ai, (size_t)Ap[n] * 8);
    std::unique_lock<std::mutex> lk(ancache::mu);
    for (;;) {
      size_t i = 0;
      while (i < ancache::entries.size() && !same(ancache::entries[i])) i++;
      if (i == ancache::entries.size()) break;
      if (!ancache::entries[i].an) { ancache::cv.wait(lk); continue; }      // being computed by another thread: wait, look again
      out = ancache::entries[i].an;
      std::rotate(ancache::entries.begin() + i, ancache::entries.begin() + i + 1, ancache::entries.end());
      return MI_OSQP_OK;
    }
    // ours to compute: a placeholder tells the others
    if (ancache::entries.size() >= ancache::kMaxEntries) {
      for (size_t i = 0; i < ancache::entries.size(); i++) if (ancache::entries[i].an) { ancache::entries.erase(ancache::entries.begin() + i); break; }
    }
    ancache::entries.push_back(ancache::Entry{hsh, n, m, nw, bt, max_extra, dt_max, tri_waves, n_tiles, tune.analysis, {Pp, Pp + n + 1}, {Pi, Pi + Pp[n]}, {Ap, Ap + n + 1}, {Ai, Ai + Ap[n]}, nullptr});
  }
  // (an exception - bad_alloc on a huge pattern - is an error like any other: the placeholder must go, or every later setup
  //  of this pattern waits for it forever)
  int rc;
  try {
    auto an = std::make_shared<Analysis>();
    rc = analyze(n, m, Pp, Pi, Ap, Ai, tune.analysis, *an, nw, bt, max_extra, dt_max, tri_waves, n_tiles);
    if (!rc) out = an;
  } catch (const std::exception &e) {
    g_last_error = std::string("pattern analysis: ") + e.what();
    rc = MI_OSQP_ERR_ALLOC;
  }
  if (use) {
    std::lock_guard<std::mutex> lk(ancache::mu);
    for (size_t i = 0; i < ancache::entries.size(); i++)
      if (!ancache::entries[i].an && same(ancache::entries[i])) {
        if (rc) ancache::entries.erase(ancache::entries.begin() + i); else ancache::entries[i].an = out;
        break;
      }
    ancache::cv.notify_all();
  }
  return rc;
}

static int refactor_qps(mi_osqp_batch *h, std::vector<int> qps);
static bool host_ruiz(const mi_osqp_batch *h);
// Kernels that spin on their own grid (the dataflow sweeps and grid barriers of a large single QP, the grouped
// refactorisation) need every workgroup of the grid resident.  The grids are clamped to what the device keeps resident
// (max_coresident_groups); two such grids on one device could still starve each other, so their launches - from any
// handle and host thread of the process - take turns per device, from the launch to its completion.
static std::mutex &spin_mutex(int device) {
  static std::mutex mu[64];
  return mu[(unsigned)device % 64u];
}
static int restore_snapshot(mi_osqp_batch *h);
static int cont_leave(mi_osqp_batch *h);      // (a blocking call ends the continuous mode of a handle: section "continuous")

// multi-workgroup mode: a grid barrier that gave up waiting (a workgroup of the grid was not resident) leaves its error
// word set; the results of that launch are garbage
static int mw_barrier_ok(mi_osqp_batch *h) {
  if (h->mw_groups <= 0) return MI_OSQP_OK;
  uint32_t w[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(w, h->mw_bar.p, sizeof(w), hipMemcpyDeviceToHost));
  if (w[2]) { g_last_error = "dataflow solve: a wait for a vector entry or a grid barrier timed out"; return MI_OSQP_ERR_DEVICE; }
  return MI_OSQP_OK;
}
// A launch that may spin on the grid of a dataflow handle, from the launch to its completion under the device's spin mutex:
// the barrier words are zeroed, `launch` enqueues on `st` (and returns a status), the stream is drained, the barrier checked.
template <class Launch>
static int run_spinning(mi_osqp_batch *h, hipStream_t st, Launch launch) {
  int rc;
  {
    std::unique_lock<std::mutex> spin_lock(spin_mutex(h->device), std::defer_lock);
    if (h->mw_groups > 0) { spin_lock.lock(); HIPCHK(hipMemsetAsync(h->mw_bar.p, 0, 4 * sizeof(uint32_t), st)); }
    if ((rc = launch())) return rc;
    HIPCHK(hipStreamSynchronize(st));
  }
  return mw_barrier_ok(h);
}

// The launch shape of a handle (threads per workgroup, QPs per tile, where the solve vector lives, the grid of a large single
// QP): what the pattern analysis is built for.  Shared by setup and by mi_osqp_prefetch_analysis.
static void derive_shape(mi_osqp_batch *h, int64_t B, int64_t n, int64_t m, int64_t device, int &BT_out, int &max_extra_out) {
  const Tuning &tu = h->tune;
  h->threads = tu.threads ? tu.threads : 512;
  // ---- tile shape (needed by the schedule layout)
  // 2 QPs per tile: iterate_kernel<2> needs 112 VGPRs, so two 512-thread workgroups share a CU and
  // cover each other's barrier stalls; measured best on the 1024-QP headline batch (4 and 1 are slower)
  int BT = tu.tile ? tu.tile : (B >= 384 ? 2 : 1);
  // vectors of 65 535 entries and more: 32-bit index words (twice the index bytes), the solve vector in global
  // memory, one QP per tile, 512 threads (the only instantiation of the wide kernels)
  const bool wide = n + m >= 65535 || 2 * n + m >= 65535;
  if (wide) { BT = 1; h->threads = std::min(h->threads, 512); }
  const size_t lds_cap = 160 * 1024 - 1024;      // (the kernels carry up to 272 B of static LDS of their own: a vector that fills
                                                 //  the 160 KB to the last byte - extra rows are handed out until it does - cannot launch)
  while (BT > 1 && lds_bytes((int)(n + m), BT, h->threads) > lds_cap) BT /= 2;
  // 16 waves per tile where a tile has its CU to itself anyway - no more tiles than CUs, or a vector of more than half the
  // LDS: 1 024 against 512 threads measured -10 % on 256 GOMP QPs (7 DOF x 100 waypoints), -18 % on 1 024 of them (2 per
  // tile, 100 KB), -4..7 % on 128-QP shards of the headline batch; the headline batch itself (512 tiles of 40 KB: two
  // 8-wave workgroups per CU cover each other's barrier stalls) stays at 8 waves
  if (!tu.threads && !wide && BT <= 2 && !tu.global_xs && lds_bytes((int)(n + m), BT, 1024) <= lds_cap) {     // (16-wave kernels: 1 or 2 QPs per tile)
    int dev = (int)device, cus = 256;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    (void)hipGetLastError();
    const int64_t tiles = (B + BT - 1) / BT;
    if (tiles <= cus || lds_bytes((int)(n + m), BT, 1024) > 80 * 1024) h->threads = 1024;
  }
  // too large for LDS even at one QP per tile: the solve vector goes to a per-tile global buffer
  h->global_xs = wide || lds_bytes((int)(n + m), BT, h->threads) > lds_cap || tu.global_xs;
  // rows that may get a second vector position (phase B of the solves): what still fits LDS (analyze() also
  // respects the 16-bit index range of the narrow index words)
  int max_extra = -1;
  if (!h->global_xs) {
    const size_t cap_rows = (lds_cap - lds_bytes(0, BT, h->threads)) / (sizeof(double) * BT);
    max_extra = (int)(cap_rows - (size_t)(n + m));
  }
  // dense tail (inverted Schur complement of the trailing rows): needs the LDS vector and <= 512 rows (one row per
  // thread of dense_inverse_kernel; k^3 flops per refactorisation)
  // one QP whose vector lives in global memory: the dataflow form of the solves, shared by several workgroups (one CU
  // cannot issue the scattered 8-byte gathers / read-modify-writes of a 10^5-row factor fast enough, and a barrier per
  // level costs more than the level: DESIGN.md 7.4).  MI_OSQP_GROUPS = 0: the barrier form, one workgroup.
  h->mw_groups = 0; h->mw_threads = 0;
  if (h->global_xs && BT == 1 && B == 1 && h->threads <= 512) {
    // measured on the 316 x 316 grid of config 5 (scripts/mw_probe.py, ms per iteration): 16 x 512 threads 1.56, 32 x 512 1.23,
    // 64 x 256 1.06, 128 x 128 1.01, 256 x 128 0.97 (the barrier form in one workgroup: 6.5); 150 x 150 grid: 128 x 128 0.40
    // (round 3, same probe: 316 x 316 grid 128 x 128 threads 0.868, 256 x 128 0.818, 192 x 128 0.823, 128 x 256 0.824, 256 x 64 0.899;
    //  150 x 150 grid: 0.371 / 0.401 / 0.387 / 0.396 / 0.394 - the larger grid for the larger QP)
    //  and smaller grids for the mid-size ones (`scripts/groups_probe.py`, ms per 25-iteration solve: the 802-waypoint trajectory QP,
    //  N = 43 284: 128 x 128 3.46, 64 x 128 3.25, 256 x 128 4.38; 402 waypoints, N = 21 684: 3.34 / 2.96, 32 x 128 2.93)
    const int64_t Nrows = n + m;
    h->mw_groups = tu.groups >= 0 ? tu.groups : (Nrows >= 250000 ? 256 : Nrows >= 60000 ? 128 : Nrows >= 30000 ? 64 : 32);
    h->mw_threads = tu.group_threads ? tu.group_threads : 128;
    if (h->mw_groups * (h->mw_threads / 64) > 2048) h->mw_groups = 2048 / (h->mw_threads / 64);
    // never more workgroups than the device keeps resident at once (their waits are for each other): the schedules are
    // built for the clamped grid; a device that cannot hold two of them gets the barrier form in one workgroup
    int dev = (int)device, cus = 0;
    if ((dev >= 0 || hipGetDevice(&dev) == hipSuccess) && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
      DevGuard guard(dev);
      if (tu.assume_cus > 0) cus = std::min(cus, tu.assume_cus);      // (tests: the clamp on a device with fewer CUs)
      const int cap = max_coresident_groups(h->mw_threads, lds_bytes(0, 1, h->threads), cus);
      if (cap > 0 && h->mw_groups > cap) h->mw_groups = cap;
      if (h->mw_groups == 1) h->mw_groups = 0;
    }
    (void)hipGetLastError();
  }
  BT_out = BT; max_extra_out = max_extra;
}

// Shape and analysis of a handle.  The shape rules above were measured on trajectory QPs (sparse chain-like factors: the
// iteration is a chain of phases, two QPs per tile share them, and with more tiles than CUs 8-wave workgroups win: 2 048 QPs of
// 6 DOF x 50 waypoints 3.6 ms per batch solve against 5.4 at one QP per tile in 16 waves).  A pattern whose analysis comes back
// with a DENSE TAIL is the other kind - its iteration streams the inverted Schur complement, i.e. bandwidth - and runs best at
// ONE QP per tile in 16-wave workgroups whatever the batch size (the headline batch, end of round 3: two per tile / 8 waves 37.6
// ms per step, one per tile / 8 waves 36.6, one per tile / 16 waves 32.0; the refactorisation packs four small tasks per wave
// at one QP per tile against two).  So such a pattern is analysed a second time for that shape (both analyses are cached).
static int shape_and_analysis(mi_osqp_batch *h, int64_t B, int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi, const int64_t *Ap,
                              const int64_t *Ai, int64_t device, int &BT, int &max_extra, std::shared_ptr<const Analysis> &out) {
  derive_shape(h, B, n, m, device, BT, max_extra);
  int rc = cached_analysis(n, m, Pp, Pi, Ap, Ai, h->tune, h->threads / 64, BT, max_extra, h->global_xs ? 0 : 512, h->mw_groups * (h->mw_threads / 64), (int)((B + BT - 1) / BT), out);
  if (rc) return rc;
  const size_t lds_cap = 160 * 1024 - 1024;
  if (out->dt.k > 0 && (BT != 1 || h->threads != 1024) && !h->global_xs && !h->tune.tile && !h->tune.threads &&
      lds_bytes((int)(n + m), 1, 1024) + (size_t)2 * 512 * sizeof(double) <= lds_cap) {
    const int BT2 = 1, thr2 = 1024;
    const size_t cap_rows = (lds_cap - lds_bytes(0, BT2, thr2)) / (sizeof(double) * BT2);
    const int max_extra2 = (int)(cap_rows - (size_t)(n + m));
    std::shared_ptr<const Analysis> an2;
    rc = cached_analysis(n, m, Pp, Pi, Ap, Ai, h->tune, thr2 / 64, BT2, max_extra2, 512, 0, (int)B, an2);
    if (!rc && an2->dt.k > 0) { BT = BT2; h->threads = thr2; max_extra = max_extra2; out = an2; }
  }
  return MI_OSQP_OK;
}

static int batch_setup_impl(mi_osqp_batch *h, int64_t B, int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi,
                            const double *Pv, const double *q, const int64_t *Ap, const int64_t *Ai,
                            const double *Av, const double *l, const double *u, int64_t device) {
  double t0 = now_s();
  if (B <= 0 || !Pp || !Ap || (m > 0 && (!l || !u)) || (Pp[n] > 0 && !Pv) || (Ap[n] > 0 && !Av)) return MI_OSQP_ERR_INVALID_DATA;
  if (validate_settings(h->st)) return MI_OSQP_ERR_INVALID_SETTINGS;
  if (h->st.adaptive_rho && !h->st.adaptive_rho_interval) {   // deterministic "auto" (upstream non-PROFILING rule)
    h->rho_interval_auto = true;
    h->st.adaptive_rho_interval = h->st.check_termination ? 4 * h->st.check_termination : 100;
  }
  for (int64_t k = 0; k < B * m; k++) if (l[k] > u[k]) return MI_OSQP_ERR_INVALID_DATA;
  int BT = 1, max_extra = -1;
  const size_t lds_cap = 160 * 1024 - 1024;
  h->tune = tuning_from_env();
  const double ta0 = now_s();
  int rc = shape_and_analysis(h, B, n, m, Pp, Pi, Ap, Ai, device, BT, max_extra, h->anp);
  const double t_analysis = now_s() - ta0;
  if (rc) return rc;
  const Analysis &an = (*h->anp);
  h->B = (int)B;
  h->failed.assign((size_t)B, 0);
  // ---- device
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_last_error = "no HIP device visible"; return MI_OSQP_ERR_DEVICE; }
  if (device >= ndev) { g_last_error = "no such HIP device"; return MI_OSQP_ERR_DEVICE; }
  if (device >= 0) h->device = (int)device; else HIPCHK(hipGetDevice(&h->device));
  DevGuard guard(h->device);            // (the caller's current device is restored when setup returns)
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, h->device));
  h->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { g_last_error = std::string("device is not gfx950: ") + prop.gcnArchName; return MI_OSQP_ERR_DEVICE; }
  {
    streampool::Bundle sb;
    const bool pooled = streampool::take(h->device, sb);
    if (pooled) {
      h->stream = sb.stream; h->ev0 = sb.ev[0]; h->ev1 = sb.ev[1]; h->evf0 = sb.ev[2]; h->evf1 = sb.ev[3]; h->evf2 = sb.ev[4];
      h->pipe_r = sb.pipe_r; h->pipe_i = sb.pipe_i; h->pipe_x = sb.pipe_x; h->pipe_c = sb.pipe_c;
      for (int k = 0; k < streampool::kPipeEvents; k++) h->pipe_ev[k] = sb.pipe_ev[k];
    }
    else {
      HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
      HIPCHK(hipEventCreate(&h->ev0)); HIPCHK(hipEventCreate(&h->ev1));
      HIPCHK(hipEventCreate(&h->evf0)); HIPCHK(hipEventCreate(&h->evf1)); HIPCHK(hipEventCreate(&h->evf2));
    }
    // MI_OSQP_REGION_PRIORITY: numerically greater = less urgent; a stream created without a priority has 0.  A form whose
    // priority is that of every other stream changes nothing and counts as not asked for (mi_osqp_stats region_priority -1).
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int asked = h->tune.region_priority;
    h->prio_inert = (asked == 1 && least == 0) || (asked == 2 && greatest == 0);
    h->prio_form = h->prio_inert ? 0 : asked;
    h->lane_prio = h->prio_form == 1 ? least : 0;
    h->chain_prio = greatest;
    // pooled lanes of another priority (idle: their handle synchronised them before it gave them back) are not handed on
    if (pooled && sb.lane_prio != h->lane_prio)
      for (hipStream_t *st : {&h->pipe_r, &h->pipe_i, &h->pipe_x}) if (*st) { (void)hipStreamDestroy(*st); *st = nullptr; }
  }
  h->BT = BT; h->ntiles = (int)((B + BT - 1) / BT);
  h->lds = h->global_xs ? lds_bytes(0, BT, h->threads) : lds_bytes(an.Next + 2 * an.dt.k, BT, h->threads);
  if (h->lds > lds_cap) { g_last_error = "internal: LDS budget exceeded"; return MI_OSQP_ERR_ALLOC; }
  // Resident state of the iterate (iterate_body RS): x, q, z, y, rho_inv, rho_vec, l, u and D^-1 of a tile stay in LDS for a
  // whole segment where they fit into what the analysis left of the cap - the extra rows it handed out are not taken back:
  // that would change the schedules, and with them the summation orders, of patterns that do not fit anyway.  Only for
  // 16-wave tiles: they have their CU's LDS to themselves, while two 8-wave tiles share a CU and would lose that.  The other
  // kernels sized by h->lds (check_kernel runs four 512-thread workgroups per CU on large batches) keep their size.
  h->lds_iter = h->lds; h->rs_off = 0;
  {
    const size_t state = sizeof(double) * (size_t)BT * (2 * (size_t)n + 6 * (size_t)m + (size_t)an.N);
    if (!h->tune.stream_state && !h->global_xs && h->mw_groups <= 0 && h->threads == 1024 && h->lds + state <= lds_cap) {
      h->rs_off = (int)(h->lds / sizeof(double)); h->lds_iter = h->lds + state;
    }
  }
  // Resident head of S^-1 (iterate_body RF): a tile of ONE QP with the resident state and a dense tail keeps the first
  // rf_head_steps(form) steps of every wave's first product task on chip across a segment - rf_lds_steps() of them in LDS behind
  // the resident state where that fits the cap as well, the rest in registers (no LDS part, no head).  The LDS part is the
  // same for both forms of the head; which one a launch runs is decided launch by launch (host_core.hpp iterate_form).
  h->lds_factor = 0; h->rf_off = 0; h->rf_steps = 0;
  if (h->rs_off && BT == 1 && an.dt.k > 0 && !h->tune.stream_factor) {
    const size_t part = (size_t)(h->threads / 64) * rf_lds_steps() * 64 * sizeof(double);
    if (h->lds_iter + part <= lds_cap) {
      h->rf_off = (int)(h->lds_iter / sizeof(double)); h->lds_factor = part;
      h->rf_steps = rf_head_steps(h->tune.rf_form == kIterDeepRing ? RF_FORM_DEEP_RING : RF_FORM_LONG_HEAD);
    }
  }
  // Index words of the resident iterate (iterate_body IX): every thread keeps its entries of pinv and xloc in registers across
  // a launch where their number fits the caps, so that the passes between the sweeps load nothing.
  h->ix = !h->tune.index_loads && index_words_fit(h->rs_off != 0, !h->global_xs, BT, h->threads, n, m) ? 1 : 0;
  // ---- device arrays
  size_t T = (size_t)h->ntiles * BT;
  if ((rc = h->fwd.upload(an.fwd)) || (rc = h->bwd.upload(an.bwd)) || (rc = h->chk.upload(an.chk))) return rc;
  { std::vector<uint32_t> pv(an.pinv.begin(), an.pinv.end()); if ((rc = h->pinv.upload(pv))) return rc; }
  { std::vector<uint32_t> xv(an.xloc.begin(), an.xloc.end()); if ((rc = h->xloc.upload(xv))) return rc; }
  {
    std::vector<int32_t> pr(an.Pi.begin(), an.Pi.begin() + an.Pp[n]), pc(an.Pp[n]), ar(an.Ai.begin(), an.Ai.begin() + an.Ap[n]), ac(an.Ap[n]);
    for (int j = 0; j < n; j++) { for (int k = an.Pp[j]; k < an.Pp[j + 1]; k++) pc[k] = j; for (int k = an.Ap[j]; k < an.Ap[j + 1]; k++) ac[k] = j; }
    if ((rc = h->rz_prow.upload(pr)) || (rc = h->rz_pcol.upload(pc)) || (rc = h->rz_arow.upload(ar)) || (rc = h->rz_acol.upload(ac))) return rc;
  }
  if ((rc = h->use_work.alloc(T)) || (rc = h->use_work.zero(h->stream))) return rc;
#define ALLOC(buf, len) if ((rc = h->buf.alloc((size_t)(len) * T)) || (rc = h->buf.zero(h->stream))) return rc
  ALLOC(fwd_val, (size_t)an.fwd.phys_steps() * 64); ALLOC(bwd_val, (size_t)an.bwd.phys_steps() * 64); ALLOC(chk_val, (size_t)an.chk.phys_steps() * 64); ALLOC(dinv, an.N);
  ALLOC(x, n); ALLOC(z, m); ALLOC(y, m); ALLOC(q, n); ALLOC(l, m); ALLOC(u, m); ALLOC(rho_vec, m); ALLOC(rho_inv, m);
  ALLOC(Dsc, n); ALLOC(Dsc_inv, n); ALLOC(Esc, m); ALLOC(Esc_inv, m); ALLOC(dx, n); ALLOC(dy, m);
  ALLOC(out1, 2 * n + m); ALLOC(out2, 2 * n + m); ALLOC(dscal, DS_COUNT);
  if (h->global_xs) { ALLOC(xs_global, an.xs_total); }
  if ((rc = h->mw_bar.alloc(4 * (size_t)std::max(h->n_cus, 1))) || (rc = h->mw_bar.zero(h->stream))) return rc;      // (one set of barrier words per work tile)
  if (an.df && ((rc = h->rflag.upload(an.rflag)) || (rc = h->mw_scratch.alloc((size_t)8 * 256 * 16)) || (rc = h->mw_scratch.zero(h->stream)))) return rc;
  if (an.dt.k) {
    const DenseTail &dt = an.dt;
    ALLOC(dt_val, (size_t)dt.n_steps * 64);
    if ((rc = h->dt_task.upload(dt.task)) || (rc = h->dt_wave_task.upload(dt.wave_task)) || (rc = h->dt_wave_step.upload(dt.wave_step)) ||
        (rc = h->dt_tail_bar.upload(dt.tail_bar)) || (rc = h->dt_src.upload(dt.src)) ||
        (rc = h->dt_lt_pos.upload(dt.lt_pos)) || (rc = h->dt_ltcol_col.upload(dt.ltcol_col)) || (rc = h->dt_tile_tab.upload(dt.tile_tab)) ||
        (rc = h->dt_wave_tiles.upload(dt.wave_tiles)) || (rc = h->dt_asm_q64.upload(dt.asm_q64)) ||
        (rc = h->dt_src_tile.upload(dt.src_tile)) || (rc = h->dt_diag_tile.upload(dt.diag_tile)) || (rc = h->dt_task_step.upload(dt.task_step)) ||
        (rc = h->dt_Sd.alloc((size_t)dt.k * dt.k * (T + 4)))) return rc;
    // LDS plan of tail_kernel: the staged half of the panel (<= 14 row tiles of 8 KiB; at least the 64 x 65 image of a pivot
    // block) + Pn in operand order (32 KiB), or the compact factor entries of the assembly phase, whichever is larger
    const int nrt = dt.k / 16 - 4;
    h->dt_nh = nrt <= 14 ? std::max(nrt, 1) : (nrt + 1) / 2;
    h->dt_cs_doubles = (uint32_t)std::max(h->dt_nh * 1024, 64 * 65 + 63) / 64 * 64;
    h->dt_lds = std::max<size_t>((size_t)h->dt_cs_doubles + 4096, 2 * 64 * 65) * sizeof(double);       // (the stream write keeps two 64 x 65 images)
    h->dt_lds_asm = (dt.asm_lds_bytes() + 255) & ~(size_t)255;
    if (h->dt_lds > lds_cap || h->dt_lds_asm > lds_cap) { g_last_error = "internal: LDS budget of tail_kernel exceeded"; return MI_OSQP_ERR_ALLOC; }
  }
#undef ALLOC
  if ((rc = h->iscal.alloc((size_t)IS_COUNT * T)) || (rc = h->flag.alloc(4))) return rc;
  {
    const BlockFactor &bf = an.bf;
    if ((rc = h->bf_blk.upload(bf.blk)) || (rc = h->bf_lvl.upload(bf.lvl)) || (rc = h->bf_ubig.upload(bf.ubig)) || (rc = h->bf_utask.upload(bf.utask4)) ||
        (rc = h->bf_tri.upload(bf.tri4)) || (rc = h->bf_dtask.upload(bf.dtask4)) || (rc = h->bf_ttask.upload(bf.ttask4)) ||
        (rc = h->bf_asm_dst.upload(bf.asm_dst)) || (rc = h->bf_asm_src.upload(bf.asm_src)) ||
        (rc = h->fwd_srcblk.upload(an.fwd_srcblk)) || (rc = h->bwd_srcblk.upload(an.bwd_srcblk))) return rc;
    if ((rc = h->pa_val.alloc((size_t)(an.Pp[n] + an.Ap[n]) * T)) || (rc = h->pa_val.zero(h->stream)) ||
        // (+4 QPs: a refactorisation may pack its work list with up to 4 QPs per workgroup, rounded up)
        (rc = h->Lblk.alloc((size_t)bf.storage * (T + 4))) || (rc = h->Dl.alloc((size_t)an.N * (T + 4))) || (rc = h->Dl.zero(h->stream)) ||
        (rc = h->dinv_scratch.alloc((size_t)an.N * (T + 4))) || (rc = h->npos.alloc(T))) return rc;
    HIPCHK(hostpool::alloc((void **)&h->h_npos, T * sizeof(int), &h->h_npos_cap));
  }
  // tables of the fused SpMV op: rows of [P x ; A'y ; A x] as (value position, vector index) pairs, 16 bits each; used
  // when the compact values of a tile and [x ; y] fit LDS together
  if (!h->global_xs && an.Pp[n] + an.Ap[n] < 65536 && n + m < 65536 &&
      spmv_fused_lds_bytes((int)n, (int)m, an.Pp[n] + an.Ap[n], BT) <= 150 * 1024) {
    const int nnzP = an.Pp[n];
    std::vector<std::vector<uint32_t>> rows((size_t)2 * n + m);
    for (int c = 0; c < (int)n; c++)
      for (int k = an.Pp[c]; k < an.Pp[c + 1]; k++) {
        const int r = an.Pi[k];
        rows[r].push_back((uint32_t)k | ((uint32_t)c << 16));
        if (r != c) rows[c].push_back((uint32_t)k | ((uint32_t)r << 16));
      }
    for (int c = 0; c < (int)n; c++)
      for (int k = an.Ap[c]; k < an.Ap[c + 1]; k++) {
        const int r = an.Ai[k];
        rows[(size_t)n + c].push_back((uint32_t)(nnzP + k) | ((uint32_t)(n + r) << 16));
        rows[(size_t)2 * n + r].push_back((uint32_t)(nnzP + k) | ((uint32_t)c << 16));
      }
    std::vector<uint32_t> ptr{0u}, ent;
    for (auto &rw : rows) { ent.insert(ent.end(), rw.begin(), rw.end()); ptr.push_back((uint32_t)ent.size()); }
    if ((rc = h->sp_ptr.upload(ptr)) || (rc = h->sp_ent.upload(ent))) return rc;
    // prefetching form
    const size_t nrows = rows.size();
    size_t maxlen = 0;
    for (auto &rw : rows) maxlen = std::max(maxlen, rw.size());
    if (nrows <= 4 * 512 && maxlen <= 24) {
      std::vector<uint32_t> order(nrows);
      for (size_t r = 0; r < nrows; r++) order[r] = (uint32_t)r;
      std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rows[x].size() > rows[y].size(); });
      const int npass = (int)((nrows + 511) / 512);
      std::vector<uint32_t> ell, rowid((size_t)npass * 512, 0xFFFFFFFFu);
      // value position of the zero, vector index of the zero slot past [x ; y] (a padding entry must not read x[0]: 0 * inf)
      const uint32_t pad = (uint32_t)(an.Pp[n] + an.Ap[n]) | ((uint32_t)(n + m) << 16);
      for (int p = 0; p < npass; p++) {
        const size_t r0 = (size_t)p * 512, r1 = std::min(nrows, r0 + 512);
        const uint32_t K = (uint32_t)rows[order[r0]].size();
        h->sp_ell_off[p] = (uint32_t)ell.size(); h->sp_ell_k[p] = K;
        ell.resize(ell.size() + (size_t)K * 512, pad);
        for (size_t r = r0; r < r1; r++) {
          rowid[r] = order[r];
          const auto &rw = rows[order[r]];
          for (size_t k = 0; k < rw.size(); k++) ell[h->sp_ell_off[p] + k * 512 + (r - r0)] = rw[k];
        }
      }
      h->sp_npass = npass;
      if ((rc = h->sp_ell.upload(ell)) || (rc = h->sp_rowid.upload(rowid))) return rc;
    }
  }
  if ((rc = h->x_out.alloc((size_t)B * n)) || (rc = h->y_out.alloc((size_t)B * std::max<int64_t>(m, 1)))) return rc;
  if ((rc = h->cert_out.alloc((size_t)B * std::max<int64_t>(std::max<int64_t>(n, m), 1)))) return rc;
  if ((rc = h->rawP.alloc((size_t)B * std::max(an.Pp[n], 1))) || (rc = h->rawq.alloc((size_t)B * n))) return rc;
  if ((rc = h->x_out.zero(h->stream)) || (rc = h->y_out.zero(h->stream)) || (rc = h->cert_out.zero(h->stream))) return rc;
  HIPCHK(hostpool::alloc((void **)&h->h_iscal, (size_t)IS_COUNT * T * sizeof(int), &h->h_iscal_cap));
  HIPCHK(hostpool::alloc((void **)&h->h_dscal, (size_t)DS_COUNT * T * sizeof(double), &h->h_dscal_cap));
  if ((rc = ensure_pin(h, std::max((size_t)2 * B * m, (size_t)B * n)))) return rc;      // (host update paths: bounds, warm starts)
  HIPCHK(hipStreamSynchronize(h->stream));
  double t1 = now_s();
  // ---- per-QP numeric (host threads), uploaded in chunks to bound host memory
  h->qp.resize(B);
  int nnzPin = (int)Pp[n], nnzA = (int)Ap[n];
  const int CH = 128;
  double t_factor = 0.0, t_upload = 0.0;
  // Row E2 (Ruiz equilibration) of a batch runs on the device (ruiz_kernel from the raw data: bit for bit what scale_qp
  // computes), like every later update of the handle; a handful of large QPs keeps the host threads (host_ruiz()).  The
  // host mirrors of the scaled problem are then fetched only if a host path ever needs them (ensure_mirrors).
  const bool dev_ruiz = !host_ruiz(h);
  for (int c0 = 0; c0 < B; c0 += CH) {
    int c1 = (int)std::min<int64_t>(B, c0 + CH);
    double ta = now_s();
    // QPs whose P, A, q equal those of the chunk's first QP (GOMP: all of them, only bounds differ) reuse its
    // equilibration.  The numeric factorisation itself happens on the device, below.
    std::vector<char> dup(c1 - c0, 0);
    std::vector<double> raw_pq((size_t)(c1 - c0) * (an.Pp[n] + n));
    for (int k = 1; k < c1 - c0 && !dev_ruiz; k++) {
      const int qi = c0 + k;
      dup[k] = !memcmp(Pv + (size_t)qi * nnzPin, Pv + (size_t)c0 * nnzPin, sizeof(double) * nnzPin) &&
               !memcmp(Av + (size_t)qi * nnzA, Av + (size_t)c0 * nnzA, sizeof(double) * nnzA) &&
               (!q || !memcmp(q + (size_t)qi * n, q + (size_t)c0 * n, sizeof(double) * n));
    }
    auto numeric = [&](int k, bool second_pass) {
      if ((bool)dup[k] != second_pass) return;
      int qi = c0 + k;
      QPNumeric &Q = h->qp[qi];
      load_qp(an, h->st, Pv + (size_t)qi * nnzPin, q ? q + (size_t)qi * n : nullptr, Av + (size_t)qi * nnzA,
              l + (size_t)qi * m, u + (size_t)qi * m, Q);
      std::copy(Q.Pv.begin(), Q.Pv.end(), raw_pq.begin() + (size_t)k * (an.Pp[n] + n));          // (before the equilibration)
      std::copy(Q.q.begin(), Q.q.end(), raw_pq.begin() + (size_t)k * (an.Pp[n] + n) + an.Pp[n]);
      if (!dev_ruiz && h->st.scaling) { if (second_pass) scale_like(an, h->qp[c0], Q); else scale_qp(an, h->st, Q); }
      set_rho_vec(an, h->st, Q);          // (device equilibration: sized here, refreshed with the mirrors)
    };
    parallel_for(c1 - c0, [&](int k, int) { numeric(k, false); });
    parallel_for(c1 - c0, [&](int k, int) { numeric(k, true); });
    double tb = now_s();
    t_factor += tb - ta;
    std::vector<int> ids(c1 - c0);
    for (int k = 0; k < c1 - c0; k++) ids[k] = c0 + k;
    if (!dev_ruiz && ((rc = upload_rho(h, ids)) || (rc = upload_problem(h, ids, true)))) return rc;
    {     // raw triu(P) and q of the chunk, QP-major (mi_osqp_batch_reinit_some; the device equilibration below)
      const size_t per = (size_t)an.Pp[n] + n;
      if ((rc = ensure_stage(h, raw_pq.size() + 1, 0))) return rc;
      HIPCHK(hipMemcpyAsync(h->stage.p, raw_pq.data(), raw_pq.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (an.Pp[n]) HIPCHK(hipMemcpy2DAsync(h->rawP.p + (size_t)c0 * an.Pp[n], (size_t)an.Pp[n] * 8, h->stage.p, per * 8, (size_t)an.Pp[n] * 8, (size_t)(c1 - c0), hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(hipMemcpy2DAsync(h->rawq.p + (size_t)c0 * n, (size_t)n * 8, h->stage.p + an.Pp[n], per * 8, (size_t)n * 8, (size_t)(c1 - c0), hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    t_upload += now_s() - tb;
  }
  {
    std::vector<int> all(B);
    for (int i = 0; i < B; i++) all[i] = i;
    size_t cnt = (size_t)DS_COUNT * T;
    for (size_t k = 0; k < cnt; k++) h->h_dscal[k] = 0.0;
    HIPCHK(hipMemcpy(h->dscal.p, h->h_dscal, cnt * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = sync_scalars_to_device(h, all, !dev_ruiz))) return rc;          // (c and 1/c belong to the equilibration)
  }
  if (dev_ruiz) {
    double tb = now_s();
    // raw A and bounds as the caller gave them (QP-major) -> ruiz_kernel in its "fresh" form -> scaled P, A, q, bounds, D, E, c
    // in the handle's layout + the scaled values once more QP-major for the check streams
    const size_t cA = (size_t)B * nnzA, cb = (size_t)B * m, cpa = (size_t)B * (an.Pp[n] + nnzA);
    if ((rc = ensure_pin(h, cA + 2 * cb + 1)) || (rc = ensure_stage(h, cA + 2 * cb + cpa + 1, (size_t)B))) return rc;
    par_copy(h->pin, Av, cA);
    if (m) { par_copy(h->pin + cA, l, cb); par_copy(h->pin + cA + cb, u, cb); }
    HIPCHK(hipMemcpyAsync(h->stage.p, h->pin, (cA + 2 * cb) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RuizArgs r{};
    r.n = (int)n; r.m = (int)m; r.nnzP = an.Pp[n]; r.nnzA = nnzA; r.B = (int)B; r.BT = BT; r.iters = (int)h->st.scaling;
    r.ids = nullptr; r.fresh = 1; r.rawP = h->rawP.p; r.rawq = h->rawq.p;
    r.Prow = h->rz_prow.p; r.Pcol = h->rz_pcol.p; r.Arow = h->rz_arow.p; r.Acol = h->rz_acol.p;
    r.rawA = h->stage.p; r.rawl = h->stage.p + cA; r.rawu = h->stage.p + cA + cb;
    r.pa_val = h->pa_val.p; r.q = h->q.p; r.Dsc = h->Dsc.p; r.Dsc_inv = h->Dsc_inv.p; r.Esc = h->Esc.p; r.Esc_inv = h->Esc_inv.p;
    r.l = h->l.p; r.u = h->u.p; r.dscal = h->dscal.p;
    r.dn = h->out1.p; r.en = h->out1.p + (size_t)B * n;
    r.pa_out = h->stage.p + cA + 2 * cb;
    HIPCHK(launch_ruiz(r, h->stream));
    std::vector<int> ids(B);
    for (int i = 0; i < (int)B; i++) ids[i] = i;
    HIPCHK(hipMemcpyAsync(h->ids.p, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(launch_scatter(r.pa_out, h->chk_val.p, h->chk.src.p, h->ids.p, (int)B, an.Pp[n] + nnzA, h->chk.view(an.chk), BT, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->host_scaling_stale = true; h->host_bounds_stale = true; h->host_rho_stale = true;
    t_factor += now_s() - tb;
  }
  // E5 numeric on the device: KKT assembly + block LDL' + inverted diagonal blocks + scatter into the solve
  // streams of every QP (the kernel every later rho / A update uses); a wrong inertia comes back as an error
  {
    double tb = now_s();
    std::vector<int> all(B);
    for (int i = 0; i < (int)B; i++) all[i] = i;
    if ((rc = refactor_qps(h, std::move(all)))) return rc;
    t_factor += now_s() - tb;
  }
  if ((rc = reset_solve_state(h, true))) return rc;
  if ((rc = snapshot(h))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  mi_osqp_stats &s = h->stats;
  s.n = n; s.m = m; s.N = an.N; s.batch = B; s.tile = BT; s.n_tiles = h->ntiles;
  s.nnz_P_triu = an.Pp[n]; s.nnz_A = nnzA; s.nnz_KKT = an.nnzK(); s.nnz_L = an.nnzL();
  s.n_supernodes = (int64_t)an.sn_start.size() - 1; s.n_blocks = (int64_t)an.chunk_start.size() - 1;
  s.fwd_levels = an.fwd.n_phases; s.bwd_levels = an.bwd.n_phases;
  s.fwd_slots = (int64_t)an.fwd.phys_steps() * 64; s.bwd_slots = (int64_t)an.bwd.phys_steps() * 64; s.chk_slots = (int64_t)an.chk.phys_steps() * 64;
  s.lds_bytes = (int64_t)h->lds; s.threads_per_block = h->threads;
  s.dense_tail_rows = an.dt.k; s.dense_tail_slots = (int64_t)an.dt.n_steps * 64;
  s.setup_seconds_host = t1 - t0; s.setup_seconds_factor = t_factor; s.setup_seconds_upload = t_upload;
  s.nnz_L_before_tail = an.dt.k ? an.Lp[an.dt.s] : an.nnzL();
  s.solve_groups = h->mw_groups; s.solve_group_threads = h->mw_groups > 0 ? h->mw_threads : 0;
  s.resident_state = h->rs_off ? 1 : 0; s.lds_bytes_iterate = (int64_t)h->lds_iter;
  s.resident_factor_steps = h->rf_steps; s.lds_bytes_factor = (int64_t)h->lds_factor;
  s.resident_index_words = h->ix;
  dense_tail_deal_stats(an.dt, s);
  if (getenv("MI_OSQP_DEBUG_TIMING"))
    fprintf(stderr, "[mi_osqp] setup B=%d N=%d: analysis+alloc %.1f ms (analysis %.1f), numeric %.1f ms, upload %.1f ms, rest %.1f ms\n", (int)B, an.N,
            1e3 * (t1 - t0), 1e3 * t_analysis, 1e3 * t_factor, 1e3 * t_upload, 1e3 * (now_s() - t1 - t_factor - t_upload));
  return MI_OSQP_OK;
}

// ------------------------------------------------------------------- solve

// Per-QP failure isolation: the slots of `bad` (slot = tile * BT + b = QP) become kNonConvex on the device
// (fail_slots_kernel) and are remembered in h->failed.
static int fail_slots(mi_osqp_batch *h, const KernelArgs &a, const std::vector<int> &bad, int iter) {
  if (bad.empty()) return 0;
  int rc;
  if (h->fail_list.n < bad.size() && (rc = h->fail_list.alloc(std::max<size_t>(bad.size(), (size_t)h->ntiles * h->BT)))) return rc;
  HIPCHK(hipMemcpyAsync(h->fail_list.p, bad.data(), bad.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(launch_fail_slots(a, h->fail_list.p, (int)bad.size(), h->BT, iter, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int q : bad) if (q >= 0 && q < h->B) h->failed[q] = 1;
  return 0;
}

// tail_assemble_kernel / tail_kernel of the ADMM factor: kbt QPs per work tile of the list `work`
static TailArgs make_tail_args(mi_osqp_batch *h, int kbt, const int *work) {
  const DenseTail &dt = (*h->anp).dt;
  TailArgs da{};
  da.n = (*h->anp).n; da.N = (*h->anp).N; da.s = dt.s; da.k = dt.k; da.kbt = kbt; da.home_bt = h->BT;
  da.storage = (*h->anp).bf.storage; da.n_slots = dt.n_steps * 64u; da.n_lt = dt.n_lt; da.n_ltcol = dt.n_ltcol; da.n_quads = (uint32_t)(dt.asm_q64.size() / 64);
  da.nh = h->dt_nh; da.cs_doubles = h->dt_cs_doubles; da.work = work;
  da.lt_pos = h->dt_lt_pos.p; da.ltcol_col = h->dt_ltcol_col.p; da.tile_tab = h->dt_tile_tab.p; da.wave_tiles = h->dt_wave_tiles.p;
  da.dt_task = h->dt_task.p; da.dt_task_step = h->dt_task_step.p; da.n_tasks = (uint32_t)(dt.task.size() / 4);
  da.asm_q64 = h->dt_asm_q64.p; da.diag_tile = h->dt_diag_tile.p; da.src_tile = h->dt_src_tile.p;
  da.Lblk = h->Lblk.p; da.Dl = h->Dl.p; da.Sd = h->dt_Sd.p; da.dt_val = h->dt_val.p; da.dinv = h->dinv.p; da.npos = h->npos.p; da.iscal = h->iscal.p;
  return da;
}

// The polish factor instead of the ADMM factor (FactorArgs::pmask; section "polish"): from the active sets of `pol`, regularised
// by delta, into the polish buffers; a wrong inertia goes to pol->stat.  da = the tail arguments of the same launch chain.
static void to_polish_factor(mi_osqp_batch *h, const PolishArgs &pol, FactorArgs &fa, TailArgs &da) {
  fa.pmask = pol.act; fa.arow = h->rz_arow.p; fa.pstat = pol.stat; fa.pdelta = h->st.delta; fa.sigma = h->st.delta;
  fa.fwd_val = h->pol_fwd.p; fa.bwd_val = h->pol_bwd.p; fa.dinv = h->pol_dinv.p; fa.use_work = nullptr;
  da.dt_val = h->pol_dt.p; da.dinv = h->pol_dinv.p; da.pstat = pol.stat;
}
// the solve arguments `a` with the polish factor's streams in place of the ADMM factor's
static KernelArgs polish_stream_args(mi_osqp_batch *h, KernelArgs a) {
  a.fwd_val = h->pol_fwd.p; a.bwd_val = h->pol_bwd.p; a.dinv = h->pol_dinv.p; a.dt_val = h->pol_dt.p; a.use_work = nullptr;
  return a;
}
// the QPs whose status word in h_iscal (the host copy of the flags) is kOptimal
static std::vector<int> koptimal_slots(const mi_osqp_batch *h) {
  const int BT = h->BT;
  std::vector<int> work;
  for (int q = 0; q < h->B; q++)
    if (h->h_iscal[(size_t)(q / BT) * IS_COUNT * BT + IS_STATUS * BT + q % BT] == 1) work.push_back(q);
  return work;
}

// Row E13 on the device for a list of slots (tile * BT + b): rho vector from the current bounds and rho, KKT
// assembly, block LDL', scatter into the solve streams.  The work list packs the slots kbt per workgroup.
// Slots whose new factor has the wrong inertia are appended to *bad (the caller isolates them).
// pol != null: the polish factor of the listed slots instead (FactorArgs::pmask; section "polish"): it goes to the polish
// buffers, leaves the ADMM factor, the rho vectors, the flags and the refactorisation statistics alone, and a wrong inertia
// only marks the slot's polish as failed.
static int device_refactor_slots(mi_osqp_batch *h, std::vector<int> work, std::vector<int> *bad, const PolishArgs *pol = nullptr) {
  if (work.empty()) return 0;
  const int BT = h->BT;
  int rc;
  FactorArgs fa = make_factor_args(h, 0);
  // QPs per workgroup of this refactorisation: one while every QP can have a CU of its own (a lone tile is
  // latency-bound: 3.3 ms with one QP, 4.6 ms with two), the solve tiling otherwise (measured: 605 QPs take
  // 10.9 ms whether packed 1, 2 or 4 per workgroup - the memory system, not the tiling, is the limit there)
  const int nq = (int)work.size();
  const int kbt = nq <= h->n_cus ? 1 : BT;
  const int wtiles = (nq + kbt - 1) / kbt;
  work.resize((size_t)wtiles * kbt, -1);
  if (h->work.n < work.size() && (rc = h->work.alloc((size_t)h->ntiles * BT + 4))) return rc;
  HIPCHK(hipMemcpyAsync(h->work.p, work.data(), work.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  fa.work = h->work.p;
  TailArgs da = make_tail_args(h, kbt, h->work.p);
  if (pol) to_polish_factor(h, *pol, fa, da);
  // Short work lists (the rho updates of the last few QPs of a batch, a strong-scaling shard, a handle with one QP): the
  // block tasks of a QP are shared by several workgroups with barriers of the group between the phases of a level
  // (3 x levels x ~6 us): one QP of config 5 (ms): 1: 275, 8: 45, 16: 28, 32: 19, 64: 15, 128: 14
  // (measured in round 3: the LDS-resident single-workgroup form of factor_kernel does NOT beat the group of workgroups on a
  //  lone QP - 0.88 against 0.43 ms at config 2: a lone QP's levels hold hundreds of block tasks, the kernel is short of
  //  waves, not of memory latency - so short lists keep their groups and the LDS form serves one-workgroup-per-QP launches)
  if (kbt == 1 && h->mw_bar.p && (*h->anp).N >= 1000) {
    const int cap = h->B == 1 ? std::max(4, std::min(64, (*h->anp).N / 600)) : 8;
    int G = h->tune.factor_groups ? h->tune.factor_groups : cap;
    G = std::min(G, std::max(1, h->n_cus / wtiles));
    static const int resident = max_coresident_factor_groups(h->tune.factor_threads, 1);      // workgroups of factor_kernel per CU
    if (resident > 0) G = std::min(G, std::max(1, resident * h->n_cus / wtiles));
    fa.mw_groups = G > 1 ? G : 0;
  }
  std::unique_lock<std::mutex> spin_lock(spin_mutex(h->device), std::defer_lock);
  if (fa.mw_groups > 1) spin_lock.lock();
  HIPCHK(hipEventRecord(h->evf0, h->stream));
  if (fa.mw_groups > 1) HIPCHK(hipMemsetAsync(h->mw_bar.p, 0, 4 * sizeof(uint32_t) * (size_t)wtiles, h->stream));
  HIPCHK(launch_factor(fa, kbt, wtiles, h->tune.factor_threads, h->stream));
  HIPCHK(hipEventRecord(h->evf1, h->stream));
  if ((*h->anp).dt.k) {      // the tail blocks now hold the Schur complement: invert it into the stream of the symmetric product
    unsigned long long *d_trace = nullptr;
    const bool tracing = getenv("MI_OSQP_TAIL_TRACE") != nullptr;          // timing stamps only; results are unaffected
    if (tracing) { HIPCHK(hipMalloc((void **)&d_trace, (size_t)wtiles * kbt * 8 * sizeof(unsigned long long))); HIPCHK(hipMemsetAsync(d_trace, 0, (size_t)wtiles * kbt * 64, h->stream)); }
    da.trace = d_trace;
    HIPCHK(launch_tail(da, wtiles * kbt, h->dt_lds_asm, h->dt_lds, h->stream));
    if (tracing) {
      std::vector<unsigned long long> tr((size_t)wtiles * kbt * 8);
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpy(tr.data(), d_trace, tr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      (void)hipFree(d_trace);
      double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (size_t i = 0; i < tr.size(); i++) sum[i % 8] += (double)tr[i] / (wtiles * kbt);
      fprintf(stderr, "[mi_osqp] tail_kernel, %d QPs, mean shader clocks of wave 0 per QP: assembly %.0f, pivot blocks %.0f, panel stores %.0f, stream write %.0f; "
              "staging %.0f, Gn %.0f, trailing %.0f, barrier waits of the panel phase %.0f\n", wtiles * kbt, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], sum[7]);
    }
  }
  HIPCHK(hipEventRecord(h->evf2, h->stream));
  HIPCHK(hipMemcpyAsync(h->h_iscal, h->iscal.p, (size_t)h->ntiles * IS_COUNT * BT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (spin_lock.owns_lock()) spin_lock.unlock();
  if (fa.mw_groups > 1) {
    std::vector<uint32_t> w(4 * (size_t)wtiles, 0u);
    HIPCHK(hipMemcpy(w.data(), h->mw_bar.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int t = 0; t < wtiles; t++)
      if (w[4 * (size_t)t + 2]) {
        // a workgroup of a group never showed up: the streams of the listed QPs hold a half-written factor.  Every listed
        // QP is without a valid factor (kNonConvex on every solve) until a later refactorisation of it succeeds.
        if (!pol) for (int sl : work) if (sl >= 0 && sl < h->B) h->failed[(size_t)sl] = 1;
        g_last_error = "refactorisation on several workgroups: a barrier of the group timed out"; return MI_OSQP_ERR_DEVICE;
      }
  }
  if (pol) return 0;
  {
    float f = 0.f, d = 0.f;
    HIPCHK(hipEventElapsedTime(&f, h->evf0, h->evf1)); HIPCHK(hipEventElapsedTime(&d, h->evf1, h->evf2));
    h->factor_ms_sum += f; h->dense_ms_sum += (*h->anp).dt.k ? d : 0.0; h->refactor_launches++; h->refactor_qps += nq;
    if (nq >= h->peak_qps) { h->peak_qps = nq; h->peak_factor_ms = f; h->peak_tail_ms = (*h->anp).dt.k ? d : 0.0; }
  }
  for (int s : work)            // (only the listed slots: at setup the flags of padding slots are not initialised yet)
    if (s >= 0 && h->h_iscal[(size_t)(s / BT) * IS_COUNT * BT + IS_NEED_REFACTOR * BT + s % BT] < 0) {
      if (getenv("MI_OSQP_DEBUG_TIMING")) {
        (void)hipMemcpy(h->h_npos, h->npos.p, (size_t)h->ntiles * BT * sizeof(int), hipMemcpyDeviceToHost);
        fprintf(stderr, "[mi_osqp] slot %d: %d positive pivots, expected %d\n", s, h->h_npos[s], (*h->anp).n);
      }
      if (bad) bad->push_back(s);
    }
  return 0;
}

// Refactorisation outside a solve (setup, update_A, constraint-type changes; slot == QP): QPs whose factor loses its
// inertia are isolated (kNonConvex on every solve until a later refactorisation of theirs succeeds); the call fails
// only when that happens to EVERY QP of the handle (a single QP: OsqpSolver::Init / the update reports the error).
static int refactor_qps(mi_osqp_batch *h, std::vector<int> qps) {
  if (qps.empty()) return 0;
  std::vector<int> bad;
  const std::vector<int> listed = qps;
  int rc = device_refactor_slots(h, std::move(qps), &bad);
  if (rc) return rc;
  for (int q : listed) h->failed[q] = 0;
  if ((rc = fail_slots(h, make_args(h), bad, 0))) return rc;
  if ((int)bad.size() == h->B) { g_last_error = "the KKT factor lost its inertia"; return MI_OSQP_ERR_NONCONVEX; }
  return 0;
}

// ------------------------------------------------------------------- polish
// the polish buffers of a handle, allocated at its first polish (the blocking polish below and mi_osqp_batch_polish_some)
static int ensure_polish_buffers(mi_osqp_batch *h) {
  if (h->pol_stat.p) return MI_OSQP_OK;
  const Analysis &an = (*h->anp);
  const size_t T = (size_t)h->ntiles * h->BT;
  int rc;
  if ((rc = h->pol_fwd.alloc(h->fwd_val.n)) || (rc = h->pol_fwd.zero(h->stream)) || (rc = h->pol_bwd.alloc(h->bwd_val.n)) ||
      (rc = h->pol_bwd.zero(h->stream)) || (rc = h->pol_dinv.alloc(h->dinv.n)) || (rc = h->pol_dinv.zero(h->stream)) ||
      (rc = h->pol_sol.alloc(T * an.N)) || (rc = h->pol_act.alloc(std::max<size_t>(1, T * an.m))) || (rc = h->pol_act.zero(h->stream)) ||
      (rc = h->pol_stat.alloc(T)) || (rc = h->pol_stat.zero(h->stream))) return rc;
  if (an.dt.k && ((rc = h->pol_dt.alloc(h->dt_val.n)) || (rc = h->pol_dt.zero(h->stream)))) return rc;
  if (!h->evp0) HIPCHK(hipEventCreate(&h->evp0));
  if (!h->evp1) HIPCHK(hipEventCreate(&h->evp1));
  return MI_OSQP_OK;
}

// Rounds of refinement against K_d behind every solve of a polish (kernels.hip reduced_solve_refine): one solve is off by up to
// 1e-3 of the solution at d = 1e-6 with a dense tail, four rounds take that below round-off.
static constexpr int kPolishInner = 4;

// Solution polishing after a blocking solve (OSQP polish.c on the scaled data): the active set of
// every kOptimal QP (polish_active_kernel), the reduced KKT matrix of those QPs factored in the handle's own pattern into
// the polish buffers (device_refactor_slots in polish mode: same work list / grouped workgroups / dense tail as a
// refactorisation), then polish_kernel: solve + refinement, projection, residuals, acceptance and write-back.  `a` = the
// solve's arguments (its x_out receives the polished solutions).  No per-QP host work beyond the work list.
static int polish_impl(mi_osqp_batch *h, const KernelArgs &a) {
  const int BT = h->BT, ntl = h->ntiles;
  int rc;
  h->pol_count = h->pol_accepted = 0; h->pol_seconds = 0.0;
  h->pol_status.assign((size_t)h->B, 0);
  if ((rc = ensure_polish_buffers(h))) return rc;
  std::vector<int> work = koptimal_slots(h);      // (h_iscal: copied at the end of the solve)
  PolishArgs pa{h->pol_stat.p, h->pol_act.p, h->pol_sol.p, (int)h->st.polish_refine_iter, kPolishInner, h->st.delta};
  HIPCHK(hipEventRecord(h->evp0, h->stream));
  HIPCHK(launch_polish_active(a, pa, BT, h->stream));
  const int n_pol = (int)work.size();
  if (n_pol) {
    if ((rc = device_refactor_slots(h, std::move(work), nullptr, &pa))) return rc;
    if ((rc = run_spinning(h, h->stream, [&]() -> int {
          HIPCHK(launch_polish(polish_stream_args(h, a), pa, BT, ntl, h->mw_groups > 0 ? h->mw_threads : h->threads, h->lds, h->n_cus, h->stream));
          HIPCHK(hipEventRecord(h->evp1, h->stream));
          return MI_OSQP_OK;
        }))) return rc;
  } else {
    HIPCHK(hipEventRecord(h->evp1, h->stream));
  }
  HIPCHK(hipMemcpyAsync(h->pol_status.data(), h->pol_stat.p, (size_t)h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->evp0, h->evp1));
  h->pol_seconds = ms * 1e-3;
  h->pol_count = n_pol;
  for (int v : h->pol_status) h->pol_accepted += v == 1;
  return MI_OSQP_OK;
}

// ------------------------------------------------------------------- adjoint
// Adjoint derivative of the solution (mi_osqp.h mi_osqp_batch_adjoint_device; DESIGN.md section 8, "Adjoint derivative"): the
// polish chain with another last kernel.  The active set of every QP whose last solve ended kOptimal from its current iterate
// (polish_active_kernel - after an accepted polish that is the polished set), the reduced KKT matrix of those QPs factored
// into the polish buffers (device_refactor_slots in polish mode), adjoint_kernel, adjoint_finish_kernel (statuses, NaN rows).
// The marks live in adj_stat, not pol_stat, and nothing a solve reads is written: the iterates, rho, the ADMM factor, the
// infos and the certificates stay as they are (out1 / pol_sol / the polish buffers are scratch of the polish as well).
static int adjoint_impl(mi_osqp_batch *h, const AdjointArgs &ga, int32_t *d_status, hipStream_t user_stream) {
  hipStream_t keep = h->stream;
  struct Restore { mi_osqp_batch *h; hipStream_t s; ~Restore() { h->stream = s; } } restore{h, keep};
  if (user_stream) h->stream = user_stream;
  const Analysis &an = (*h->anp);
  const int BT = h->BT, ntl = h->ntiles;
  int rc;
  if ((rc = ensure_polish_buffers(h))) return rc;
  if (!h->adj_stat.p && ((rc = h->adj_stat.alloc((size_t)ntl * BT)))) return rc;
  if ((rc = h->adj_stat.zero(h->stream))) return rc;
  std::vector<int> work;                // the QPs whose last solve ended kOptimal
  if (h->solved_once) {                 // (before that the status words are not initialised; the continuous mode sets it too)
    HIPCHK(hipMemcpyAsync(h->h_iscal, h->iscal.p, (size_t)ntl * IS_COUNT * BT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    work = koptimal_slots(h);
  }
  if (!work.empty()) {
    const KernelArgs a = make_args(h);
    PolishArgs pa{h->adj_stat.p, h->pol_act.p, h->pol_sol.p, (int)h->st.polish_refine_iter};
    HIPCHK(launch_polish_active(a, pa, BT, h->stream));
    if ((rc = device_refactor_slots(h, std::move(work), nullptr, &pa))) return rc;
    if ((rc = run_spinning(h, h->stream, [&]() -> int {
          HIPCHK(launch_adjoint(polish_stream_args(h, a), pa, ga, BT, ntl, h->mw_groups > 0 ? h->mw_threads : h->threads, h->lds, h->n_cus, h->stream));
          return MI_OSQP_OK;
        }))) return rc;
  }
  HIPCHK(launch_adjoint_finish(h->adj_stat.p, ga, d_status, h->B, an.n, an.m, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MI_OSQP_OK;
}

// ------------------------------------------------ pipelined refactorisation
// A long work list at a rho-update point ("Pipelined refactorisation"): no tile shares anything with
// another, so a tile may start the next segment as soon as the factors of its own QPs are written.  The work list is cut into
// chunks (host_core.hpp refactor_chunks).  Stream R runs factor_kernel -> tail_assemble_kernel -> tail_kernel chunk after chunk
// with an event behind each; stream I runs iterate_kernel over the tiles of a chunk (KernelArgs::tiles) once that chunk's event
// has fired - chunk 0, the tiles without a flagged QP, at once.  Both fork from the solve stream and join it again, so callers
// see the ordering they always saw.  Only ordinary LDS-vector batches: no launch here spins on other workgroups.
// Chunk lanes (MI_OSQP_REFACTOR_LANES > 1; host_core.hpp refactor_lanes): up to three streams that each run the whole chain
// factor -> tail -> iterate of their chunks, so the drain of one chain's kernel is filled by the other chains.  Chunks on
// different lanes run side by side: each keeps its block storage / D / Schur scratch at its own offset of the work list
// (FactorArgs / TailArgs wg_base); a tile of several QPs whose flagged QPs sit in chunks of different lanes waits for the
// other lanes' tail events.  The events are recorded in ascending chunk order on the host, so every wait sees its record.
// Behind the join fail_flagged_kernel ends the slots whose new factor lost its inertia; the host learns of them from the flag
// copy behind the check that follows (pipelined_region_finish) - no host turn between the region and that check.
struct PipeRegion {
  bool open = false;
  int iter = 0, n_chunks = 0, n_lanes = 1;
  bool tail = false;
  int chk_threads = 0;                // in: threads of the solve loop's check launches (the lanes' own checks take the same)
  bool lane_checks = false;           // the lanes have failed and checked their own chunks: no check_kernel launch behind the join
  double host_s = 0.0;                // host time up to the fork
  std::vector<int> work, wl, tiles;   // the flagged slots; the lists the copies read
  std::vector<int> lane_last;         // per lane: its last refactorisation chunk (0: none)
};
// the defaults of MI_OSQP_REFACTOR_LANES / MI_OSQP_REFACTOR_CHUNK0 (measured, DESIGN.md section 4: two lanes beat three at the
// headline batch - three chains of equal chunks run in lockstep, factor beside factor, tail beside tail, and overlap nothing)
constexpr int kDefaultLanes = 2;
constexpr bool kDefaultChunk0First = false;
static bool pipeline_applies(const mi_osqp_batch *h, int n_ref) {
  const int longer_than = h->tune.pipeline_min > 0 ? h->tune.pipeline_min : h->n_cus;
  return h->tune.refactor_pipeline && n_ref > longer_than && h->mw_groups <= 0 && !h->global_xs && !(*h->anp).wide && !(*h->anp).df;
}

// ---- run-ahead ("Run-ahead"): the last few QPs of a batch need several segments more than everyone else,
// and a lone tile's segment is a latency chain that leaves the other CUs idle.  At a pipelined rho-update point the tiles
// furthest from convergence (host_core.hpp runahead_group, from the residuals the check has just stored: KernelArgs::res) leave
// the region: their flagged slots leave its work list, their tiles its chunks.  They run as a chain on the solve stream - idle
// until the join otherwise - beside the lanes and past them, without a host turn: factor -> tail -> fail_flagged of the
// group's flagged slots,
// then per segment iterate_kernel + check_kernel over the group's tile list and, at a rho-update point inside the chain,
// worklist_of_kernel -> factor -> tail -> fail_flagged over a device-built list (grid = the group; a workgroup whose entry is
// -1 leaves at once).  The chain ends at the rho-update point after next or at max_iter - without a refactorisation there -
// and the waits for the lanes follow it.  (A stream of its own for the chain was measured first: a fifth stream of the
// process shares a hardware queue with a lane, and the chain then waits for that lane's kernels - DESIGN.md section 4.)
// Every QP sees the same kernels on the same data in the same order as without
// run-ahead; only when it runs changes.  The scratch of the chain's refactorisations sits behind the region's in the scratch
// buffers (wg_base): the region's flagged slots and the group's tiles are different QPs, so both fit.
// One QP per tile and at most two chunk lanes only (with the chain three streams run side by side), once per solve.
struct RunAhead {
  bool open = false;                    // a chain is enqueued and the host has not read its flags yet
  bool used = false;                    // this solve has sent a group ahead
  int chk_threads = 0;                  // threads of the check launches (those of the solve's other checks)
  std::vector<int> points;              // the ends of the chain's segments; back() = where the chain ends
  std::vector<int> group, rest, work;   // the group's tiles in descending score; every other tile, ascending; the group's flagged slots
  std::vector<int> ru0;                 // IS_RHO_UPDATES of the group's QPs in front of the chain
};
// the default of MI_OSQP_RUNAHEAD_TILES in quarters of the CU count (measured among 64, 128 and 192 tiles at the headline batch,
// DESIGN.md section 4; half the CUs held every late QP of that batch in the oracle's residuals)
constexpr int kRunaheadQuarters = 2;
static bool runahead_applies(const mi_osqp_batch *h) {
  const int lanes = h->tune.refactor_lanes > 0 ? h->tune.refactor_lanes : kDefaultLanes;
  return h->tune.runahead && h->tune.refactor_pipeline && h->BT == 1 && lanes <= 2 && h->st.adaptive_rho && h->st.adaptive_rho_interval > 0 &&
         h->mw_groups <= 0 && !h->global_xs && !(*h->anp).wide && !(*h->anp).df;
}
static int ensure_runahead_buffers(mi_osqp_batch *h) {
  int rc;
  if (!h->ra_list.p && (rc = h->ra_list.alloc((size_t)5 * h->ntiles))) return rc;
  if (!h->ra_res.p && (rc = h->ra_res.alloc((size_t)2 * h->ntiles))) return rc;
  if (!h->h_res) HIPCHK(hostpool::alloc((void **)&h->h_res, (size_t)2 * h->ntiles * sizeof(double), &h->h_res_cap));
  if (!h->h_mark) HIPCHK(hostpool::alloc((void **)&h->h_mark, (size_t)h->ntiles * sizeof(int), &h->h_mark_cap));
  return 0;
}

// Enqueues the refactorisation of the slots of `work`, iterations (a.iter_begin, a.iter_end] of the tiles that hold a slot of
// `active` and, behind the join, the failure of the slots whose new factor has the wrong inertia (their iterate left them
// alone, tile_ptrs) at iteration a.iter_begin.  Nothing is synchronised: the caller enqueues the check, reads the flags and
// calls pipelined_region_finish.  Accounting: see mi_osqp_batch_last_solve_stats / DESIGN.md section 4.
// ra != null: `work` and `active` are without the run-ahead group *ra, whose chain is enqueued beside the region.
static int pipelined_refactor_iterate(mi_osqp_batch *h, const KernelArgs &a, const std::vector<int> &work, const std::vector<int> &active, PipeRegion *pr,
                                      const RunAhead *ra = nullptr) {
  using streampool::kPipeChunks; using streampool::kPipeEvents; using streampool::kPipeLanes;
  const double t_begin = now_s();
  const int BT = h->BT, nq = (int)work.size();
  int rc;
  // a lane of the handle's lane priority (MI_OSQP_REGION_PRIORITY = 1: the least one - wherever a CU frees up, the workgroups
  // of the chain on the solve stream go first)
  auto lane_stream = [&](hipStream_t *st) -> int {
    if (*st) return 0;
    if (h->lane_prio != 0) HIPCHK(hipStreamCreateWithPriority(st, hipStreamNonBlocking, h->lane_prio));
    else HIPCHK(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    return 0;
  };
  if ((rc = lane_stream(&h->pipe_r)) || (rc = lane_stream(&h->pipe_i))) return rc;
  for (int k = 0; k < kPipeEvents; k++) if (!h->pipe_ev[k]) HIPCHK(hipEventCreate(&h->pipe_ev[k]));
  hipEvent_t ev_fork = h->pipe_ev[0], ev_i0 = h->pipe_ev[1], ev_join = h->pipe_ev[2], ev_chain = h->pipe_ev[kPipeEvents - 1];
  auto ev_chunk = [&](int c, int k) { return h->pipe_ev[3 + 3 * (c - 1) + k]; };      // chunk c >= 1; k = 0 begin, 1 factor done, 2 tail done
  auto ev_lane = [&](int l) { return h->pipe_ev[3 + 3 * kPipeChunks + l]; };          // end of lane l (one lane: of stream I)
  // default (host_core.hpp region_chunk_qps): the fewest even chunks that are one round of one-workgroup-per-QP kernels each,
  // the chain's refactorisation counted with them (headline batch, 605 QPs on 256 CUs: 3 x 202 beat 2 x 303, 4 x 152, 6 x 101
  // and 256 + 256 + 93; 496 QPs beside a chain of 107: DESIGN.md section 4)
  const int cus = h->tune.assume_cus > 0 ? std::min(h->n_cus, h->tune.assume_cus) : h->n_cus;
  int chunk_qps = region_chunk_qps(nq, ra ? (int)ra->work.size() : 0, cus, kPipeChunks);
  if (h->tune.pipeline_chunks > 0) chunk_qps = (nq + h->tune.pipeline_chunks - 1) / h->tune.pipeline_chunks;
  if (h->tune.pipeline_chunks <= 0 && h->tune.pipeline_chunk_qps > 0) chunk_qps = h->tune.pipeline_chunk_qps;
  const RefactorChunks ch = refactor_chunks(work, active, BT, chunk_qps, kPipeChunks);
  // the work list chunk after chunk, each packed kbt slots per workgroup (as device_refactor_slots packs the whole list)
  const int kbt = nq <= h->n_cus ? 1 : BT;
  const int lanes_asked = h->tune.refactor_lanes > 0 ? h->tune.refactor_lanes : kDefaultLanes;
  const RefactorLanes rl = refactor_lanes(ch, work, BT, kbt, std::min(lanes_asked, kPipeLanes), h->tune.lanes_chunk0 < 0 ? kDefaultChunk0First : h->tune.lanes_chunk0 != 0,
                                          h->ntiles * BT + 4);      // (what Lblk, Dl, dinv_scratch and dt_Sd hold: setup)
  const int L = rl.n_lanes;
  if (L > 2 && (rc = lane_stream(&h->pipe_x))) return rc;
  if (ra && (L > 2 || BT != 1)) { g_last_error = "run-ahead beside three chunk lanes / tiles of several QPs"; return MI_OSQP_ERR_INVALID_SETTINGS; }
  // MI_OSQP_REGION_PRIORITY = 2: the chain on a stream of its own at the greatest priority
  const bool chain_high = ra && h->prio_form == 2;
  if (chain_high && !h->pipe_c) HIPCHK(hipStreamCreateWithPriority(&h->pipe_c, hipStreamNonBlocking, h->chain_prio));
  // MI_OSQP_LANE_CHECKS (one-QP tiles): behind the tail of a chunk fail_flagged_kernel over that chunk's list, behind its
  // iterate check_kernel over its tiles - the order of the chain below - and only the flag copy behind the join
  const bool lane_checks = h->tune.lane_checks && BT == 1;
  std::vector<int> &wl = pr->wl;
  std::vector<int> wl_begin(1, 0);
  wl.clear();
  for (int c = 1; c < ch.n_chunks; c++) {
    wl.insert(wl.end(), work.begin() + ch.work_begin[c], work.begin() + ch.work_begin[c + 1]);
    wl.resize((wl.size() + kbt - 1) / kbt * kbt, -1);
    wl_begin.push_back((int)wl.size());
  }
  pr->tiles = ch.tiles; pr->work = work;
  if (h->work.n < wl.size() && (rc = h->work.alloc((size_t)h->ntiles * BT + 4 + (size_t)BT * kPipeChunks))) return rc;
  if (h->tile_list.n < ch.tiles.size() && (rc = h->tile_list.alloc((size_t)h->ntiles))) return rc;
  HIPCHK(hipMemcpyAsync(h->work.p, wl.data(), wl.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tile_list.p, pr->tiles.data(), pr->tiles.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  // the lists of the run-ahead chain (mi_osqp_batch::ra_list; ensure_runahead_buffers has run)
  const int ntl = h->ntiles, G = ra ? (int)ra->group.size() : 0, gw = ra ? (int)ra->work.size() : 0;
  int *d_rest = h->ra_list.p, *d_group = d_rest + ntl, *d_gwork = d_rest + 2 * (size_t)ntl, *d_dwork = d_rest + 3 * (size_t)ntl, *d_mark = d_rest + 4 * (size_t)ntl;
  if (ra) {
    if (!h->ra_list.p || G <= 0 || G + (int)ra->rest.size() != ntl || gw > G || nq + G > ntl + 4) { g_last_error = "run-ahead: inconsistent lists"; return MI_OSQP_ERR_INVALID_SETTINGS; }
    if (!ra->rest.empty()) HIPCHK(hipMemcpyAsync(d_rest, ra->rest.data(), ra->rest.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_group, ra->group.data(), (size_t)G * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (gw) HIPCHK(hipMemcpyAsync(d_gwork, ra->work.data(), (size_t)gw * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(d_mark, 0, (size_t)ntl * sizeof(int), h->stream));
  }
  pr->host_s = now_s() - t_begin;
  HIPCHK(hipEventRecord(ev_fork, h->stream));
  FactorArgs fa = make_factor_args(h, 0);
  const bool tail = (*h->anp).dt.k != 0;
  // factor_kernel -> tail_assemble_kernel -> tail_kernel of chunk c >= 1 on stream st, its scratch at slot `base` of the scratch buffers
  auto enqueue_refactor = [&](int c, int base, hipStream_t st) -> int {
    const int *wc = h->work.p + wl_begin[c - 1];
    const int slots = wl_begin[c] - wl_begin[c - 1];
    fa.work = wc; fa.wg_base = base / kbt;
    HIPCHK(hipEventRecord(ev_chunk(c, 0), st));
    HIPCHK(launch_factor(fa, kbt, slots / kbt, h->tune.factor_threads, st));
    HIPCHK(hipEventRecord(ev_chunk(c, 1), st));
    if (tail) {
      TailArgs da = make_tail_args(h, kbt, wc);
      da.wg_base = base;
      HIPCHK(launch_tail(da, slots, h->dt_lds_asm, h->dt_lds, st));
    }
    // (in front of the event: whoever waits for this chunk's factors iterates its tiles, and a failed slot is finished by then)
    if (lane_checks) HIPCHK(launch_fail_flagged(a, wc, slots, BT, a.iter_begin, st));
    HIPCHK(hipEventRecord(ev_chunk(c, 2), st));
    return 0;
  };
  KernelArgs ai = a;
  auto enqueue_iterate = [&](int c, hipStream_t st) -> int {
    const int nt = ch.tile_begin[c + 1] - ch.tile_begin[c];
    if (!nt) return 0;
    ai.tiles = h->tile_list.p + ch.tile_begin[c];
    ai.rf_form = iterate_form(nt, h->rf_off != 0, h->tune);
    h->rf_launches[ai.rf_form]++;
    HIPCHK(launch_iterate(ai, BT, nt, h->threads, h->lds_iter + h->lds_factor, st));
    // the solve loop's check of this segment (device_turn: the same arguments, thread count included), over this chunk's tiles
    if (lane_checks) HIPCHK(launch_check(ai, BT, nt, pr->chk_threads, h->lds, st));
    return 0;
  };
  // ---- the run-ahead chain on the solve stream, which has nothing else to do until the join: its first refactorisation and
  // segment are enqueued in front of the region's launches (the chain is the longer path), the rest behind them and in front
  // of the waits of the join
  // (MI_OSQP_REGION_PRIORITY = 2: on pipe_c, forked like a lane behind the list copies and joined with the lanes)
  hipStream_t sx = chain_high ? h->pipe_c : h->stream;
  if (chain_high) HIPCHK(hipStreamWaitEvent(sx, ev_fork, 0));
  KernelArgs ac = a;
  ac.tiles = d_group; ac.res = nullptr; ac.info_at_end = 1;
  FactorArgs fg = make_factor_args(h, 0);
  fg.wg_base = nq;                      // behind the scratch of the region's whole work list (kbt = 1: a slot per workgroup)
  auto chain_refactor = [&](const int *list, int n, int iter) -> int {
    if (n <= 0) return 0;
    fg.work = list;
    HIPCHK(launch_factor(fg, 1, n, h->tune.factor_threads, sx));
    if (tail) {
      TailArgs da = make_tail_args(h, 1, list);
      da.wg_base = nq;
      HIPCHK(launch_tail(da, n, h->dt_lds_asm, h->dt_lds, sx));
    }
    HIPCHK(launch_fail_flagged(a, list, n, BT, iter, sx, d_mark));
    return 0;
  };
  auto chain_segment = [&](size_t k) -> int {
    ac.iter_begin = k ? ra->points[k - 1] : a.iter_begin; ac.iter_end = ra->points[k];
    ac.rf_form = iterate_form(G, h->rf_off != 0, h->tune);
    h->rf_launches[ac.rf_form]++;
    HIPCHK(launch_iterate(ac, BT, G, h->threads, h->lds_iter + h->lds_factor, sx));
    HIPCHK(launch_check(ac, BT, G, ra->chk_threads, h->lds, sx));
    const int e = ra->points[k];
    if (k + 1 < ra->points.size() && e % (int)h->st.adaptive_rho_interval == 0) {      // a rho-update point inside the chain
      HIPCHK(launch_worklist_of(h->iscal.p, d_group, d_dwork, G, BT, sx));
      return chain_refactor(d_dwork, G, e);
    }
    return 0;
  };
  if (ra) {
    if ((rc = chain_refactor(d_gwork, gw, a.iter_begin)) || (rc = chain_segment(0))) return rc;
  }
  pr->lane_last.assign(L, 0);
  if (L == 1) {
    HIPCHK(hipStreamWaitEvent(h->pipe_r, ev_fork, 0));
    HIPCHK(hipStreamWaitEvent(h->pipe_i, ev_fork, 0));
    // ---- stream R
    for (int c = 1; c < ch.n_chunks; c++) if ((rc = enqueue_refactor(c, 0, h->pipe_r))) return rc;
    pr->lane_last[0] = ch.n_chunks - 1;
    // ---- stream I
    HIPCHK(hipEventRecord(ev_i0, h->pipe_i));
    for (int c = 0; c < ch.n_chunks; c++) {
      if (c) HIPCHK(hipStreamWaitEvent(h->pipe_i, ev_chunk(c, 2), 0));
      if ((rc = enqueue_iterate(c, h->pipe_i))) return rc;
    }
    // ---- join (stream I has waited for every chunk of R)
    HIPCHK(hipEventRecord(ev_lane(0), h->pipe_i));
  } else {
    hipStream_t lane[kPipeLanes] = {h->pipe_r, h->pipe_i, h->pipe_x};
    for (int l = 0; l < L; l++) HIPCHK(hipStreamWaitEvent(lane[l], ev_fork, 0));
    const bool chunk0_first = rl.order[rl.lane_of[0]].front() == 0;
    if (chunk0_first && (rc = enqueue_iterate(0, lane[rl.lane_of[0]]))) return rc;
    size_t w = 0;         // (the waits are sorted by the waiting chunk)
    for (int c = 1; c < ch.n_chunks; c++) {
      const int l = rl.lane_of[c];
      if ((rc = enqueue_refactor(c, rl.scratch_begin[c], lane[l]))) return rc;
      pr->lane_last[l] = c;
      for (; w < rl.wait_chunk.size() && rl.wait_chunk[w] == c; w++) HIPCHK(hipStreamWaitEvent(lane[l], ev_chunk(rl.wait_for[w], 2), 0));
      if ((rc = enqueue_iterate(c, lane[l]))) return rc;
    }
    if (!chunk0_first && (rc = enqueue_iterate(0, lane[rl.lane_of[0]]))) return rc;
    // ---- join
    for (int l = 0; l < L; l++) HIPCHK(hipEventRecord(ev_lane(l), lane[l]));
  }
  if (ra) for (size_t k = 1; k < ra->points.size(); k++) if ((rc = chain_segment(k))) return rc;      // the rest of the chain
  if (chain_high) { HIPCHK(hipEventRecord(ev_chain, sx)); HIPCHK(hipStreamWaitEvent(h->stream, ev_chain, 0)); }
  for (int l = 0; l < L; l++) HIPCHK(hipStreamWaitEvent(h->stream, ev_lane(l), 0));
  HIPCHK(hipEventRecord(ev_join, h->stream));
  // a rho update that makes the factor lose its inertia ends THAT QP as kNonConvex ([EXT] osqp_solve: adapt_rho fails ->
  // OSQP_NON_CVX, break); every other QP of the batch goes on
  if (!lane_checks) HIPCHK(launch_fail_flagged(a, h->work.p, (int)wl.size(), BT, a.iter_begin, h->stream));
  pr->open = true; pr->iter = a.iter_begin; pr->n_chunks = ch.n_chunks; pr->n_lanes = L; pr->tail = tail; pr->lane_checks = lane_checks;
  h->refactor_lanes = std::max<int64_t>(h->refactor_lanes, L);
  h->region_priority = h->prio_inert ? -1 : h->prio_form;
  h->region_lane_checks = lane_checks; h->region_chunks = ch.n_chunks - 1;
  return 0;
}

// Behind the synchronisation that follows the region's check: its accounting from the events, and the slots fail_flagged_kernel
// ended (status kNonConvex in the flag copy h_iscal) into h->failed.
static int pipelined_region_finish(mi_osqp_batch *h, PipeRegion *pr) {
  using streampool::kPipeChunks;
  if (!pr->open) return 0;
  pr->open = false;
  const int BT = h->BT, nq = (int)pr->work.size();
  hipEvent_t ev_fork = h->pipe_ev[0], ev_i0 = h->pipe_ev[1], ev_join = h->pipe_ev[2];
  auto ev_chunk = [&](int c, int k) { return h->pipe_ev[3 + 3 * (c - 1) + k]; };
  float f_ms = 0.f, d_ms = 0.f, r_ms = 0.f, i_ms = 0.f, w_ms = 0.f;
  for (int c = 1; c < pr->n_chunks; c++) {
    float f = 0.f, d = 0.f;
    HIPCHK(hipEventElapsedTime(&f, ev_chunk(c, 0), ev_chunk(c, 1))); HIPCHK(hipEventElapsedTime(&d, ev_chunk(c, 1), ev_chunk(c, 2)));
    f_ms += f; d_ms += pr->tail ? d : 0.f;
  }
  for (int c : pr->lane_last) {         // the latest tail-done event of any lane
    float r = 0.f;
    if (c) HIPCHK(hipEventElapsedTime(&r, ev_fork, ev_chunk(c, 2)));
    r_ms = std::max(r_ms, r);
  }
  HIPCHK(hipEventElapsedTime(&w_ms, ev_fork, ev_join));
  // the span of the iterates as one launch (it contains waiting): of stream I, or with lanes - an iterate on some lane from
  // the first chunk's tail on at the latest, chunk 0 from the fork on - of the whole region
  if (pr->n_lanes == 1) HIPCHK(hipEventElapsedTime(&i_ms, ev_i0, h->pipe_ev[3 + 3 * kPipeChunks])); else i_ms = w_ms;
  // refactor_s: up to the last tail event; device_s: what remained exposed of the iterate, up to the join - together the wall time
  // (lane checks: the tail event of a chunk lies behind its fail_flagged_kernel, and the lanes' checks lie in front of the join -
  // the segment's check, which the other form launches behind the join and nobody accounts for, is part of device_s)
  const double wall = pr->host_s + 1e-3 * std::max(w_ms, r_ms), ref_s = pr->host_s + 1e-3 * r_ms;
  h->last_refactor_s += ref_s; h->last_device_s += wall - ref_s;
  h->kernel_ms_sum += i_ms; h->kernel_launches++; h->last_launches++;
  h->factor_ms_sum += f_ms; h->dense_ms_sum += d_ms; h->refactor_launches++; h->refactor_qps += nq;
  if (nq >= h->peak_qps) { h->peak_qps = nq; h->peak_factor_ms = f_ms; h->peak_tail_ms = d_ms; }
  h->pipelined_refactors++;
  for (int s : pr->work)
    if (s >= 0 && s < h->B && h->h_iscal[(size_t)(s / BT) * IS_COUNT * BT + IS_STATUS * BT + s % BT] == -7) h->failed[s] = 1;
  return 0;
}

// The ADMM loop runs in segments that end at every termination-check / rho-update
// point: iterate_kernel (E6-E10) -> check_kernel (E11-E14) -> host reads the flags,
// runs the device refactorisation for the QPs whose rho changed, and continues.
// (a long work list: the refactorisation and the iterate of the next segment are pipelined, pipelined_refactor_iterate)
static int solve_impl(mi_osqp_batch *h, double *d_x_out, hipStream_t user_stream) {
  hipStream_t keep = h->stream;
  struct Restore { mi_osqp_batch *h; hipStream_t s; ~Restore() { h->stream = s; } } restore{h, keep};
  if (user_stream) h->stream = user_stream;
  int rc;
  if ((rc = reset_solve_state(h, !h->st.warm_start))) return rc;
  KernelArgs a = make_args(h);
  if (d_x_out) a.x_out = d_x_out;
  h->last_total_iters = h->last_launches = h->last_refactors = 0;
  h->last_device_s = h->last_refactor_s = 0.0;
  const int BT = h->BT, ntl = h->ntiles, nslots = ntl * BT;
  const Settings &S = h->st;
  int iterating = ntl;        // tiles the next launch will actually iterate (the others leave at once): picks its form
  {     // QPs without a valid factor (isolated earlier) are kNonConvex from the start
    std::vector<int> bad;
    for (int q = 0; q < h->B; q++) if (h->failed[q]) bad.push_back(q);
    if ((rc = fail_slots(h, a, bad, 0))) return rc;
  }
  auto segment_end = [&](int iter) {       // the next termination-check / rho-update point after iteration `iter`
    int seg_end = (int)S.max_iter;
    if (S.check_termination > 0) seg_end = std::min<int64_t>(seg_end, (iter / S.check_termination + 1) * S.check_termination);
    if (S.adaptive_rho && S.adaptive_rho_interval > 0)
      seg_end = std::min<int64_t>(seg_end, (iter / S.adaptive_rho_interval + 1) * S.adaptive_rho_interval);
    return seg_end;
  };
  // run-ahead (above pipelined_refactor_iterate): the checks of this solve store the residuals of the running QPs
  const int ra_min = h->tune.runahead_min > 0 ? h->tune.runahead_min : h->n_cus;
  if (runahead_applies(h) && ntl > 1 && ntl >= ra_min) {
    if ((rc = ensure_runahead_buffers(h))) return rc;
    a.res = h->ra_res.p;
  }
  auto is_rho_point = [&](int iter) { return S.adaptive_rho && S.adaptive_rho_interval > 0 && iter % S.adaptive_rho_interval == 0; };
  auto loop = [&]() -> int {
    int iter = 0;
    bool iterated = false;       // the segment's iterations have run already, pipelined with the refactorisation before them
    PipeRegion region;           // ... and this is that region, enqueued and not yet accounted for
    // run-ahead: the group whose chain is enqueued beside the region.  Behind the chain the launches serve the tiles of a list
    // (d_tiles, n_launch of them) and the host looks at the slots that are not held: first everyone but the members the chain
    // left - at its end, or finished there at max_iter with a rho update to refactor - then those alone (`left`, ascending).
    RunAhead ra;
    std::vector<char> held;
    std::vector<int> left;
    const int *d_tiles = nullptr;
    int n_launch = ntl, res_iter = -1;
    bool leftovers_phase = false;
    auto check_threads = [&]() {
      // The check of more 16-wave tiles than the CUs hold at once (two each) runs in 8-wave workgroups - four per CU, one round
      // instead of two; the check schedule is walked stream by stream by however many waves there are, row by row in the
      // same order (headline batch: 0.19 -> 0.11 ms per check, 31.8 -> 31.5 ms per step).
      int chk_threads = h->mw_groups > 0 ? h->mw_threads : h->threads;
      if (h->mw_groups <= 0 && h->threads == 1024 && ntl > 2 * h->n_cus) chk_threads = 512;
      return chk_threads;
    };
    // ---- one segment on the device: iterations (iter, seg_end] unless a region has run them, the check, the flags to the host
    auto device_turn = [&](int seg_end) -> int {
      a.iter_begin = iter; a.iter_end = seg_end; a.info_at_end = 1; a.tiles = d_tiles;
      {
        std::unique_lock<std::mutex> spin_lock(spin_mutex(h->device), std::defer_lock);
        if (h->mw_groups > 0) spin_lock.lock();
        if (!iterated) {
          HIPCHK(hipEventRecord(h->ev0, h->stream));
          if (h->mw_groups > 0) HIPCHK(hipMemsetAsync(h->mw_bar.p, 0, 4 * sizeof(uint32_t), h->stream));
          a.rf_form = iterate_form(iterating, h->rf_off != 0, h->tune);
          h->rf_launches[a.rf_form]++;
          HIPCHK(launch_iterate(a, BT, n_launch, h->mw_groups > 0 ? h->mw_threads : h->threads, h->lds_iter + h->lds_factor, h->stream));
          HIPCHK(hipEventRecord(h->ev1, h->stream));
        }
        // (a region whose lanes checked their own chunks has run this check already, tile list by tile list)
        if (!(iterated && region.open && region.lane_checks)) HIPCHK(launch_check(a, BT, n_launch, check_threads(), h->lds, h->stream));
        HIPCHK(hipMemcpyAsync(h->h_iscal, h->iscal.p, (size_t)ntl * IS_COUNT * BT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        // run-ahead: the residuals of the running QPs behind the check of a rho-update point (a group may be chosen from them);
        // behind a chain the marks of the slots it failed
        if (a.res && !ra.used && is_rho_point(seg_end) && seg_end < S.max_iter) {
          HIPCHK(hipMemcpyAsync(h->h_res, h->ra_res.p, (size_t)2 * ntl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
          res_iter = seg_end;
        }
        if (ra.open) HIPCHK(hipMemcpyAsync(h->h_mark, h->ra_list.p + 4 * (size_t)ntl, (size_t)ntl * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
      }
      if ((rc = mw_barrier_ok(h))) {
        // waves that gave up waiting have consumed "not yet" patterns: x, y, z (and with them every later warm start) are
        // garbage.  Back to the last good state: the factor / rho of the snapshot, cold iterates.
        const std::string why = g_last_error;
        (void)restore_snapshot(h);
        g_last_error = why + " (the handle is back in the state of its last setup / update, cold-started)";
        return rc;
      }
      if (!iterated) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        h->last_device_s += ms * 1e-3; h->kernel_ms_sum += ms; h->kernel_launches++; h->last_launches++;
      } else if ((rc = pipelined_region_finish(h, &region))) return rc;
      iterated = false;
      if (ra.open) {
        // Behind the chain: its members are finished or at the chain's end.  The refactorisations inside the chain are the
        // rho updates the members have counted since, less those the chain's last check asked for (the host runs them, with
        // the leftovers); the slots the chain failed are marked; who is left waits for the others to finish.
        ra.open = false;
        int64_t inner = 0, n_left = 0;
        for (size_t i = 0; i < ra.group.size(); i++) {
          const int t = ra.group[i];
          const int *f = h->h_iscal + (size_t)t * IS_COUNT;
          const bool flagged = f[IS_NEED_REFACTOR] == 1;
          inner += f[IS_RHO_UPDATES] - ra.ru0[i] - (flagged ? 1 : 0);
          if (h->h_mark[t]) h->failed[(size_t)t] = 1;
          n_left += !f[IS_DONE];
          if (!f[IS_DONE] || flagged) left.push_back(t);
        }
        std::sort(left.begin(), left.end());
        h->last_refactors += inner; h->refactor_qps += (int64_t)ra.work.size() + inner;
        h->ra_left += n_left;
        if (left.empty()) { d_tiles = nullptr; n_launch = ntl; }
        else { held.assign((size_t)nslots, 0); for (int t : left) held[(size_t)t] = 1; }
      }
      return 0;
    };
    // ---- the host's turn behind a check at iteration `iter`, from the flags in h_iscal: who goes on (*go_on: anybody), and
    // row E13 on the device for the QPs whose rho changed - serially, or as a region pipelined with the next segment
    auto host_turn = [&](bool *go_on) -> int {
      *go_on = false;
      // QPs still iterating / asking for a refactorisation.  A QP that runs into max_iter at a rho-update iteration
      // has finished AND asks for its refactorisation: upstream adapts rho (and refactors) before it leaves the loop,
      // and the next Solve() of a warm-started solver continues from that factor.
      std::vector<int> active, work;
      for (int s = 0; s < h->B; s++) {
        if (!held.empty() && held[(size_t)s]) continue;
        const int *t = h->h_iscal + (size_t)(s / BT) * IS_COUNT * BT;
        if (!t[IS_DONE * BT + s % BT]) active.push_back(s);
        if (t[IS_NEED_REFACTOR * BT + s % BT]) work.push_back(s);
      }
      // run-ahead counter: who outside the group is still active after the segment that follows the region
      if (ra.used && !leftovers_phase && ra.points.size() && iter == segment_end(ra.points[0])) h->ra_missed += (int64_t)active.size();
      const int n_ref = (int)work.size();
      if (active.empty() && !n_ref) return 0;
      // ---- row E13 on the device: rho vector, KKT assembly, block LDL', scatter into the schedules
      if (n_ref) {
        double tr = now_s();
        std::vector<int> bad;             // QPs whose refactorisation lost the inertia
        int rc2;
        // work list: the flagged QPs of the whole batch (fewer, fuller tiles = fewer rounds over the CUs)
        if (!active.empty() && pipeline_applies(h, n_ref)) {
          // a long list: its chunks overlap with the next segment's iterations, chunk after chunk
          KernelArgs nx = a;
          nx.iter_begin = iter; nx.iter_end = segment_end(iter); nx.info_at_end = 1;
          // run-ahead: the group among the active tiles, from the residuals this point's check stored; it goes ahead when the
          // rest of the work list is still a pipelined one
          std::vector<int> work_m, active_m;
          region.chk_threads = check_threads();
          if (a.res && !ra.used && res_iter == iter) {
            std::vector<double> pri(active.size()), dua(active.size());
            for (size_t i = 0; i < active.size(); i++) { pri[i] = h->h_res[2 * (size_t)active[i]]; dua[i] = h->h_res[2 * (size_t)active[i] + 1]; }
            const int size = h->tune.runahead_tiles > 0 ? h->tune.runahead_tiles : std::max(1, h->n_cus * kRunaheadQuarters / 4);
            std::vector<int> group = runahead_group(active, pri, dua, size, ra_min);
            if (!group.empty() && group.size() < active.size()) {
              std::vector<char> in((size_t)nslots, 0);
              for (int t : group) in[(size_t)t] = 1;
              for (int s : work) (in[(size_t)s] ? ra.work : work_m).push_back(s);
              for (int s : active) if (!in[(size_t)s]) active_m.push_back(s);
              if (pipeline_applies(h, (int)work_m.size())) {
                for (int t = 0; t < ntl; t++) if (!in[(size_t)t]) ra.rest.push_back(t);
                for (int t : group) ra.ru0.push_back(h->h_iscal[(size_t)t * IS_COUNT + IS_RHO_UPDATES]);
                const int interval = (int)S.adaptive_rho_interval;
                const int end = (int)std::min<int64_t>(S.max_iter, (int64_t)(iter / interval + 2) * interval);
                for (int it = iter; it < end && (h->tune.runahead_end <= 0 || (int)ra.points.size() < h->tune.runahead_end);) ra.points.push_back(it = segment_end(it));
                ra.group = std::move(group); ra.chk_threads = check_threads();
                ra.used = ra.open = true;
              } else ra.work.clear();
            }
          }
          if (ra.open) {
            if ((rc2 = pipelined_refactor_iterate(h, nx, work_m, active_m, &region, &ra))) return rc2;
            d_tiles = h->ra_list.p; n_launch = (int)ra.rest.size();       // the region's check and what follows leave the group alone
            h->ra_regions++; h->ra_tiles += (int64_t)ra.group.size();
          } else if ((rc2 = pipelined_refactor_iterate(h, nx, work, active, &region))) return rc2;
          iterated = true;
          tr = now_s();         // (the region does its own accounting, and fails the QPs that lost their inertia on the device)
        } else if ((rc2 = device_refactor_slots(h, std::move(work), &bad))) return rc2;
        // a rho update that makes the factor lose its inertia ends THAT QP as kNonConvex ([EXT] osqp_solve: adapt_rho
        // fails -> OSQP_NON_CVX, break); every other QP of the batch goes on
        if ((rc2 = fail_slots(h, a, bad, iter))) return rc2;
        h->host_rho_stale = true;
        h->last_refactors += n_ref;
        h->last_refactor_s += now_s() - tr;
        if (!bad.empty()) {
          std::vector<char> isbad(nslots, 0);
          for (int q : bad) isbad[q] = 1;
          active.erase(std::remove_if(active.begin(), active.end(), [&](int q) { return isbad[q] != 0; }), active.end());
        }
      }
      if (active.empty()) return 0;
      iterating = 0;
      for (size_t i = 0; i < active.size(); i++) iterating += !i || active[i] / BT != active[i - 1] / BT;
      *go_on = true;
      return 0;
    };
    while (true) {
      const int seg_end = segment_end(iter);
      if ((rc = device_turn(seg_end))) return rc;
      iter = seg_end;
      bool go_on = false;
      if ((rc = host_turn(&go_on))) return rc;
      if (go_on) continue;
      // nobody is active any more: on with the members the chain left, alone, from the iteration their chain ended at - the
      // flags the host holds are theirs still (nothing has touched them since the chain), so the host's turn comes first
      if (leftovers_phase || left.empty()) break;
      leftovers_phase = true;
      held.assign((size_t)nslots, 1);
      for (int t : left) held[(size_t)t] = 0;
      HIPCHK(hipMemcpyAsync(h->ra_list.p, left.data(), left.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
      d_tiles = h->ra_list.p; n_launch = (int)left.size();
      a.tiles = d_tiles;
      iter = ra.points.back();
      if ((rc = host_turn(&go_on))) return rc;
      if (!go_on) break;
    }
    return MI_OSQP_OK;
  };
  rc = loop();
  a.tiles = nullptr; a.res = nullptr;
  if (rc) {
    if (h->pipe_r) (void)hipStreamSynchronize(h->pipe_r);
    if (h->pipe_i) (void)hipStreamSynchronize(h->pipe_i);
    if (h->pipe_x) (void)hipStreamSynchronize(h->pipe_x);
    if (h->pipe_c) (void)hipStreamSynchronize(h->pipe_c);
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  HIPCHK(hipMemcpyAsync(h->h_iscal, h->iscal.p, (size_t)nslots * IS_COUNT * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int qi = 0; qi < h->B; qi++)
    h->last_total_iters += h->h_iscal[(size_t)(qi / BT) * IS_COUNT * BT + IS_ITER * BT + qi % BT];
  h->solved_once = true;
  if (h->st.polish && (rc = polish_impl(h, a))) return rc;
  if (!h->st.polish) { h->pol_status.clear(); h->pol_count = h->pol_accepted = 0; }      // (what polish_some left: every QP has been solved again)
  return MI_OSQP_OK;
}

// ---------------------------------------------------------------- C entry points

extern "C" {

void mi_osqp_default_settings(mi_osqp_settings *s) {
  if (!s) return;
  s->rho = 0.1; s->sigma = 1e-6; s->scaling = 10; s->adaptive_rho = 1; s->adaptive_rho_interval = 0;
  s->adaptive_rho_tolerance = 5.0; s->max_iter = 4000; s->eps_abs = 1e-3; s->eps_rel = 1e-3;
  s->eps_prim_inf = 1e-4; s->eps_dual_inf = 1e-4; s->alpha = 1.6; s->scaled_termination = 0;
  s->check_termination = 25; s->warm_start = 1; s->verbose = 0;
  s->polish = 0; s->polish_refine_iter = 3; s->delta = 1e-6;
}

const char *mi_osqp_exit_code_name(int64_t c) {
  static const char *names[] = {"kOptimal", "kPrimalInfeasible", "kDualInfeasible", "kOptimalInaccurate",
                                "kPrimalInfeasibleInaccurate", "kDualInfeasibleInaccurate", "kMaxIterations",
                                "kInterrupted", "kTimeLimitReached", "kNonConvex", "kUnknown"};
  return (c >= 0 && c <= 10) ? names[c] : "kUnknown";
}
const char *mi_osqp_error_name(int64_t e) {
  static const char *names[] = {"ok", "invalid data", "invalid settings", "sparsity pattern changed",
                                "non-convex problem / KKT inertia", "device error", "null argument", "allocation / size"};
  return (e >= 0 && e <= 7) ? names[e] : "unknown";
}
const char *mi_osqp_version(void) { return "mi-osqp 0.2 (gfx950)"; }
const char *mi_osqp_last_error(void) { return g_last_error.c_str(); }

static int64_t exit_code_of(int status) {
  switch (status) {
    case 1: return MI_OSQP_EXIT_OPTIMAL;
    case 2: return MI_OSQP_EXIT_OPTIMAL_INACCURATE;
    case -3: return MI_OSQP_EXIT_PRIMAL_INFEASIBLE;
    case 3: return MI_OSQP_EXIT_PRIMAL_INFEASIBLE_INACCURATE;
    case -4: return MI_OSQP_EXIT_DUAL_INFEASIBLE;
    case 4: return MI_OSQP_EXIT_DUAL_INFEASIBLE_INACCURATE;
    case -2: return MI_OSQP_EXIT_MAX_ITERATIONS;
    case -5: return MI_OSQP_EXIT_INTERRUPTED;
    case -6: return MI_OSQP_EXIT_TIME_LIMIT_REACHED;
    case -7: return MI_OSQP_EXIT_NON_CONVEX;
    default: return MI_OSQP_EXIT_UNKNOWN;
  }
}

int mi_osqp_batch_setup(mi_osqp_batch **out, int64_t B, int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi,
                        const double *Pv, const double *q, const int64_t *Ap, const int64_t *Ai, const double *Av,
                        const double *l, const double *u, const mi_osqp_settings *settings, int64_t device) {
  CallTimer timer_("batch_setup");
  if (!out) return MI_OSQP_ERR_NULL;
  *out = nullptr;
  if (n <= 0 || m < 0) return MI_OSQP_ERR_INVALID_DATA;
  mi_osqp_batch *h = new (std::nothrow) mi_osqp_batch();
  if (!h) return MI_OSQP_ERR_ALLOC;
  h->st = to_settings(settings);
  int rc = batch_setup_impl(h, B, n, m, Pp, Pi, Pv, q, Ap, Ai, Av, l, u, device);
  if (rc) { delete h; return rc; }
  *out = h;
  return MI_OSQP_OK;
}

// The pattern analysis a later setup of B QPs with this pattern on this device will ask for, computed now into the
// process-wide cache (a planner that knows its coming patterns - the ten horizons of a GOMP run - calls this from spare
// host threads; a setup that arrives while it is still running waits for it instead of computing it twice).
int mi_osqp_prefetch_analysis(int64_t B, int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi, const int64_t *Ap, const int64_t *Ai, int64_t device) {
  CallTimer timer_("prefetch_analysis");
  if (B <= 0 || n <= 0 || m < 0 || !Pp || !Ap || (Pp[n] > 0 && !Pi) || (Ap[n] > 0 && !Ai)) return MI_OSQP_ERR_INVALID_DATA;
  mi_osqp_batch tmp;
  tmp.tune = tuning_from_env();
  int BT = 1, max_extra = -1;
  std::shared_ptr<const Analysis> an;
  return shape_and_analysis(&tmp, B, n, m, Pp, Pi, Ap, Ai, device, BT, max_extra, an);
}

void mi_osqp_batch_free(mi_osqp_batch *h) { delete h; }
void mi_osqp_release_device_cache(void) { devpool::release_all(); hostpool::release_all(); streampool::release_all(); }

int mi_osqp_batch_solve(mi_osqp_batch *h) {
  CallTimer timer_("batch_solve");
  if (!h) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const int rc = solve_impl(h, nullptr, nullptr);
  if (CallTimer::on() && getenv("MI_OSQP_DEBUG_SOLVES"))
    fprintf(stderr, "[mi_osqp] solve B=%d N=%d: %ld segments of <= 25 iterations, %.0f QP-iterations in total, iterate %.2f ms, refactor %.2f ms (%ld)\n", h->B,
            (*h->anp).N, (long)h->last_launches, (double)h->last_total_iters, 1e3 * h->last_device_s, 1e3 * h->last_refactor_s, (long)h->last_refactors);
  return rc;
}

int mi_osqp_batch_solve_device(mi_osqp_batch *h, double *d_x_out, int32_t *d_status, int32_t *d_iters, void *stream) {
  if (!h) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  int rc = solve_impl(h, d_x_out, (hipStream_t)stream);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (d_x_out) {   // keep the internal copy coherent for get_primal()
    HIPCHK(hipMemcpyAsync(h->x_out.p, d_x_out, (size_t)h->B * (*h->anp).n * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  if (d_status || d_iters) HIPCHK(launch_gather_status(h->iscal.p, d_status, d_iters, h->B, h->BT, s));
  HIPCHK(hipStreamSynchronize(s));
  return MI_OSQP_OK;
}

int mi_osqp_batch_get_primal(mi_osqp_batch *h, double *x) {
  CallTimer timer_("batch_get_primal");
  if (!h || !x) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  HIPCHK(hipMemcpy(x, h->x_out.p, (size_t)h->B * (*h->anp).n * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OSQP_OK;
}
int mi_osqp_batch_get_dual(mi_osqp_batch *h, double *y) {
  if (!h || !y) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  if ((*h->anp).m) HIPCHK(hipMemcpy(y, h->y_out.p, (size_t)h->B * (*h->anp).m * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OSQP_OK;
}

// Infeasibility certificates (mi_osqp.h).  check_body stores the certificate of a QP whose solve ends infeasible into its
// row of cert_out and nothing for any other QP; which rows hold a certificate of the asked kind is read from the exit codes
// of the last finished solves, and every other row of the answer is NaN-filled here, on the host.
static bool cert_status(int64_t status, bool primal) { return primal ? (status == -3 || status == 3) : (status == -4 || status == 4); }
static void cert_row(double *dst, const double *src, size_t len, bool valid) {
  if (valid) memcpy(dst, src, len * sizeof(double));
  else std::fill(dst, dst + len, std::numeric_limits<double>::quiet_NaN());
}
static int get_cert(mi_osqp_batch *h, double *out, bool primal) {
  CallTimer timer_(primal ? "batch_get_prim_inf_cert" : "batch_get_dual_inf_cert");
  if (!h || !out) return MI_OSQP_ERR_NULL;
  const size_t n = (size_t)(*h->anp).n, m = (size_t)(*h->anp).m, len = primal ? m : n, stride = std::max(std::max(n, m), (size_t)1);
  if (!len) return MI_OSQP_OK;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const int BT = h->BT;
  HIPCHK(hipMemcpy(h->h_iscal, h->iscal.p, (size_t)h->ntiles * IS_COUNT * BT * sizeof(int), hipMemcpyDeviceToHost));
  auto status = [&](int q) { return h->h_iscal[(size_t)(q / BT) * IS_COUNT * BT + IS_STATUS * BT + q % BT]; };
  // the buffer is fetched only when a QP holds a certificate of this kind (the usual batch has none: NaN rows, no copy)
  bool any = false;
  for (int q = 0; q < h->B && !any; q++) any = cert_status(status(q), primal);
  std::vector<double> rows;
  if (any) {
    rows.resize((size_t)h->B * stride);
    HIPCHK(hipMemcpy(rows.data(), h->cert_out.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  for (int q = 0; q < h->B; q++) {
    const bool valid = any && cert_status(status(q), primal);
    cert_row(out + (size_t)q * len, valid ? rows.data() + (size_t)q * stride : nullptr, len, valid);
  }
  return MI_OSQP_OK;
}
int mi_osqp_batch_get_prim_inf_cert(mi_osqp_batch *h, double *dy_out) { return get_cert(h, dy_out, true); }
int mi_osqp_batch_get_dual_inf_cert(mi_osqp_batch *h, double *dx_out) { return get_cert(h, dx_out, false); }

// the report of QP q as the host images h_iscal / h_dscal hold it (the caller has fetched them)
static void info_from_images(const mi_osqp_batch *h, int q, mi_osqp_info &I) {
  const int BT = h->BT, b = q % BT;
  const int *ti = h->h_iscal + (size_t)(q / BT) * IS_COUNT * BT;
  const double *td = h->h_dscal + (size_t)(q / BT) * DS_COUNT * BT;
  I.iter = ti[IS_ITER * BT + b]; I.status_val = ti[IS_STATUS * BT + b]; I.exit_code = exit_code_of((int)I.status_val);
  I.obj_val = td[DS_OBJ * BT + b]; I.pri_res = td[DS_PRI_RES * BT + b]; I.dua_res = td[DS_DUA_RES * BT + b];
  I.rho_updates = ti[IS_RHO_UPDATES * BT + b]; I.rho_estimate = td[DS_RHO_EST * BT + b]; I.rho = td[DS_RHO * BT + b];
  I.status_polish = h->pol_status.empty() ? 0 : h->pol_status[(size_t)q];
}

int mi_osqp_batch_get_info(mi_osqp_batch *h, mi_osqp_info *info) {
  CallTimer timer_("batch_get_info");
  if (!h || !info) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  size_t icnt = (size_t)h->ntiles * IS_COUNT * h->BT, dcnt = (size_t)h->ntiles * DS_COUNT * h->BT;
  HIPCHK(hipMemcpy(h->h_iscal, h->iscal.p, icnt * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(h->h_dscal, h->dscal.p, dcnt * sizeof(double), hipMemcpyDeviceToHost));
  for (int q = 0; q < h->B; q++) info_from_images(h, q, info[q]);
  return MI_OSQP_OK;
}

int mi_osqp_batch_last_polish_stats(mi_osqp_batch *h, int64_t *polished, int64_t *accepted, double *seconds) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (polished) *polished = h->pol_count;
  if (accepted) *accepted = h->pol_accepted;
  if (seconds) *seconds = h->pol_seconds;
  return MI_OSQP_OK;
}

int mi_osqp_batch_get_polish_active(mi_osqp_batch *h, int8_t *act) {
  if (!h || !act) return MI_OSQP_ERR_NULL;
  const size_t cnt = (size_t)h->B * (*h->anp).m;
  if (!h->pol_act.p) { memset(act, 0, cnt); return MI_OSQP_OK; }
  DevGuard guard(h->device);
  if (h->cont.on) HIPCHK(hipStreamSynchronize(h->stream));      // (polish_some only enqueues; the continuous mode goes on)
  if (cnt) HIPCHK(hipMemcpy(act, h->pol_act.p, cnt, hipMemcpyDeviceToHost));
  return MI_OSQP_OK;
}

// Adjoint derivative (mi_osqp.h; section "adjoint" above).  Refusals come before anything is enqueued.
static AdjointArgs adjoint_args(mi_osqp_batch *h, const double *d_dx, const double *d_dy, double *d_dq, double *d_dP, double *d_dA,
                                double *d_dl, double *d_du) {
  const Analysis &an = (*h->anp);
  AdjointArgs ga{};
  ga.gx = d_dx; ga.gy = d_dy; ga.dq = d_dq; ga.dP = d_dP; ga.dA = d_dA; ga.dl = d_dl; ga.du = d_du;
  ga.prow = h->rz_prow.p; ga.pcol = h->rz_pcol.p; ga.arow = h->rz_arow.p; ga.acol = h->rz_acol.p;
  ga.nnzP = (int)an.Pp[an.n]; ga.nnzA = (int)an.Ap[an.n];
  return ga;
}
int mi_osqp_batch_adjoint_device(mi_osqp_batch *h, const double *d_dx, const double *d_dy, double *d_dq, double *d_dP, double *d_dA,
                                 double *d_dl, double *d_du, int32_t *d_status, void *stream) {
  CallTimer timer_("batch_adjoint_device");
  if (!h) return MI_OSQP_ERR_NULL;
  if (!d_dx) { g_last_error = "adjoint: dx is null (dL/dx is required; only dy may be null)"; return MI_OSQP_ERR_NULL; }
  for (const double *o : {(const double *)d_dq, (const double *)d_dP, (const double *)d_dA, (const double *)d_dl, (const double *)d_du})
    if (o && (o == d_dx || o == d_dy)) { g_last_error = "adjoint: an output aliases dx or dy"; return MI_OSQP_ERR_INVALID_DATA; }
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  return adjoint_impl(h, adjoint_args(h, d_dx, d_dy, d_dq, d_dP, d_dA, d_dl, d_du), d_status, (hipStream_t)stream);
}
int mi_osqp_batch_adjoint(mi_osqp_batch *h, const double *dx, const double *dy, double *dq, double *dP, double *dA, double *dl,
                          double *du, int32_t *status) {
  CallTimer timer_("batch_adjoint");
  if (!h) return MI_OSQP_ERR_NULL;
  if (!dx) { g_last_error = "adjoint: dx is null (dL/dx is required; only dy may be null)"; return MI_OSQP_ERR_NULL; }
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const Analysis &an = (*h->anp);
  const size_t B = (size_t)h->B, n = (size_t)an.n, m = (size_t)an.m, nnzP = (size_t)an.Pp[an.n], nnzA = (size_t)an.Ap[an.n];
  // one device block: dx, dy, then the requested outputs
  const size_t len[7] = {B * n, dy ? B * m : 0, dq ? B * n : 0, dP ? B * nnzP : 0, dA ? B * nnzA : 0, dl ? B * m : 0, du ? B * m : 0};
  size_t off[8] = {0};
  for (int k = 0; k < 7; k++) off[k + 1] = off[k] + len[k];
  DevBuf<double> buf;
  DevBuf<int> stat;
  int rc;
  if ((rc = buf.alloc(off[7])) || (rc = stat.alloc(B))) return rc;
  auto at = [&](int k) -> double * { return len[k] ? buf.p + off[k] : nullptr; };
  HIPCHK(hipMemcpy(at(0), dx, len[0] * sizeof(double), hipMemcpyHostToDevice));
  if (len[1]) HIPCHK(hipMemcpy(at(1), dy, len[1] * sizeof(double), hipMemcpyHostToDevice));
  if ((rc = adjoint_impl(h, adjoint_args(h, at(0), at(1), at(2), at(3), at(4), at(5), at(6)), stat.p, nullptr))) return rc;
  double *out[7] = {nullptr, nullptr, dq, dP, dA, dl, du};
  for (int k = 2; k < 7; k++) if (len[k]) HIPCHK(hipMemcpy(out[k], at(k), len[k] * sizeof(double), hipMemcpyDeviceToHost));
  if (status) HIPCHK(hipMemcpy(status, stat.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  return MI_OSQP_OK;
}

// The scaling the kernels use: the device copies Dsc, Esc and DS_C of dscal, out of the tile layout (the host mirrors
// h->qp[q] lag behind after a device equilibration).
int mi_osqp_batch_get_scaling(mi_osqp_batch *h, double *D, double *E, double *c) {
  if (!h || !D || !E || !c) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const int n = (*h->anp).n, m = (*h->anp).m, B = h->B, BT = h->BT;
  int rc;
  if ((rc = ensure_stage(h, (size_t)B * std::max({n, m, 1}) + 1, 0))) return rc;
  auto down = [&](const double *src, int len, double *dst) -> int {
    if (!len) return 0;
    HIPCHK(launch_deinterleave(src, h->stage.p, B, len, BT, h->stream));
    HIPCHK(hipMemcpyAsync(dst, h->stage.p, (size_t)B * len * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  };
  if ((rc = down(h->Dsc.p, n, D)) || (rc = down(h->Esc.p, m, E))) return rc;
  const size_t dcnt = (size_t)h->ntiles * DS_COUNT * BT;
  HIPCHK(hipMemcpy(h->h_dscal, h->dscal.p, dcnt * sizeof(double), hipMemcpyDeviceToHost));
  for (int q = 0; q < B; q++) c[q] = h->h_dscal[(size_t)(q / BT) * DS_COUNT * BT + DS_C * BT + q % BT];
  return MI_OSQP_OK;
}

int mi_osqp_batch_get_stats(mi_osqp_batch *h, mi_osqp_stats *st) {
  if (!h || !st) return MI_OSQP_ERR_NULL;
  *st = h->stats;
  st->pipelined_refactors = h->pipelined_refactors;
  st->refactor_lanes = h->refactor_lanes;
  st->iterate_launches_deep_ring = h->rf_launches[RF_FORM_DEEP_RING];
  st->iterate_launches_long_head = h->rf_launches[RF_FORM_LONG_HEAD];
  st->runahead_regions = h->ra_regions; st->runahead_tiles = h->ra_tiles;
  st->runahead_left = h->ra_left; st->runahead_missed = h->ra_missed;
  st->region_priority = h->region_priority; st->region_lane_checks = h->region_lane_checks; st->region_chunks = h->region_chunks;
  return MI_OSQP_OK;
}

int mi_osqp_batch_get_ordering(mi_osqp_batch *h, int64_t *kkt_perm) {
  if (!h || !kkt_perm) return MI_OSQP_ERR_NULL;
  const Analysis &an = (*h->anp);
  for (int k = 0; k < an.N; k++) kkt_perm[k] = an.perm[(size_t)k];
  return MI_OSQP_OK;
}

int mi_osqp_batch_last_solve_stats(mi_osqp_batch *h, int64_t *total_iters, int64_t *kernel_launches, double *device_seconds,
                                   double *refactor_seconds, int64_t *refactor_count, double *compact_seconds) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (compact_seconds) *compact_seconds = 0.0;      // (the QPs are not compacted during a solve; the field stays in the ABI)
  if (total_iters) *total_iters = h->last_total_iters;
  if (kernel_launches) *kernel_launches = h->last_launches;
  if (device_seconds) *device_seconds = h->last_device_s;
  if (refactor_seconds) *refactor_seconds = h->last_refactor_s;
  if (refactor_count) *refactor_count = h->last_refactors;
  return MI_OSQP_OK;
}

int mi_osqp_batch_kernel_time(mi_osqp_batch *h, double *avg_ms, int64_t *launches) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (avg_ms) *avg_ms = h->kernel_launches ? h->kernel_ms_sum / (double)h->kernel_launches : 0.0;
  if (launches) *launches = h->kernel_launches;
  h->kernel_ms_sum = 0.0; h->kernel_launches = 0;
  return MI_OSQP_OK;
}

int mi_osqp_batch_refactor_time(mi_osqp_batch *h, double *factor_ms, double *dense_ms, int64_t *launches, int64_t *qps) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (factor_ms) *factor_ms = h->factor_ms_sum;
  if (dense_ms) *dense_ms = h->dense_ms_sum;
  if (launches) *launches = h->refactor_launches;
  if (qps) *qps = h->refactor_qps;
  h->factor_ms_sum = h->dense_ms_sum = 0.0; h->refactor_launches = h->refactor_qps = 0;
  h->peak_qps = 0; h->peak_factor_ms = h->peak_tail_ms = 0.0;
  return MI_OSQP_OK;
}

int mi_osqp_batch_refactor_peak(mi_osqp_batch *h, int64_t *qps, double *factor_ms, double *tail_ms) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (qps) *qps = h->peak_qps;
  if (factor_ms) *factor_ms = h->peak_factor_ms;
  if (tail_ms) *tail_ms = h->peak_tail_ms;
  return MI_OSQP_OK;
}

int mi_osqp_batch_reset(mi_osqp_batch *h) {
  CallTimer timer_("batch_reset");
  if (!h) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  return restore_snapshot(h);
}
}  // extern "C"
// the state right after setup / the last update that refactored: factor, rho vectors and scalars of the snapshot, cold iterates
static int restore_snapshot(mi_osqp_batch *h) {
  h->clear_rho_updates = true;
  auto cp = [&](DevBuf<double> &dst, DevBuf<double> &src) -> int {
    if (src.n) HIPCHK(hipMemcpyAsync(dst.p, src.p, src.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
  };
  int rc;
  const size_t nflags = (size_t)h->ntiles * h->BT;
  // every QP's factor is its snapshot again: one word per QP instead of 1 GB of stream copies at the headline batch
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->use_work.p, 0, nflags, h->stream));
  if ((rc = cp(h->dinv, h->dinv0)) || (rc = cp(h->rho_vec, h->rho_vec0)) || (rc = cp(h->rho_inv, h->rho_inv0)) || (rc = cp(h->dscal, h->dscal0))) return rc;
  if ((rc = reset_solve_state(h, true))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  // the host mirrors of rho follow the snapshot lazily (sync_rho_to_host, only the host update paths need them)
  h->host_rho_stale = true;
  return MI_OSQP_OK;
}
extern "C" {

int mi_osqp_batch_warm_start_x(mi_osqp_batch *h, const double *x) {
  CallTimer timer_("batch_warm_start_x");
  if (!h || !x) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  h->st.warm_start = 1;
  size_t cnt = (size_t)h->B * (*h->anp).n;
  int rc;
  if ((rc = ensure_stage(h, cnt, 0)) || (rc = ensure_pin(h, cnt))) return rc;
  par_copy(h->pin, x, cnt);
  HIPCHK(hipMemcpyAsync(h->stage.p, h->pin, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KernelArgs a = make_args(h);
  HIPCHK(launch_warm_start(a, h->BT, h->ntiles, h->threads, h->lds, h->stream, h->stage.p));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MI_OSQP_OK;
}

static int update_bounds_on_host(mi_osqp_batch *h, const double *l, const double *u);
static int ensure_mirrors(mi_osqp_batch *h);
static int update_bounds_on_device(mi_osqp_batch *h, const double *d_l, const double *d_u, hipStream_t s, const double *h_l, const double *h_u);

int mi_osqp_batch_update_bounds(mi_osqp_batch *h, const double *l, const double *u) {
  CallTimer timer_("batch_update_bounds");
  if (!h || !l || !u) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  // through pinned memory to the device, where the rows are scaled and checked (bounds_kernel); only when a row changes
  // its type (equality / inequality / free: new rho vector, new factor) the host mirrors take over
  const size_t cnt = (size_t)h->B * (*h->anp).m;
  if (!cnt) return MI_OSQP_OK;
  int rc;
  if ((rc = ensure_stage(h, 2 * cnt, 0)) || (rc = ensure_pin(h, 2 * cnt))) return rc;
  {
    // in slices of 4 MB: the transfer of one runs while the host threads copy the next (as in device_update)
    const size_t slice = (size_t)1 << 19;
    for (int part = 0; part < 2; part++) {
      const double *src = part ? u : l;
      for (size_t o = 0; o < cnt; o += slice) {
        const size_t len = std::min(slice, cnt - o), off = (size_t)part * cnt + o;
        par_copy(h->pin + off, src + o, len);
        HIPCHK(hipMemcpyAsync(h->stage.p + off, h->pin + off, len * sizeof(double), hipMemcpyHostToDevice, h->stream));
      }
    }
  }
  return update_bounds_on_device(h, h->stage.p, h->stage.p + cnt, h->stream, l, u);
}

static int update_bounds_on_host(mi_osqp_batch *h, const double *l, const double *u) {
  { int rc0 = ensure_mirrors(h); if (rc0) return rc0; }
  h->clear_rho_updates = true;
  const Analysis &an = (*h->anp);
  int m = an.m, B = h->B, rc;
  for (size_t k = 0; k < (size_t)B * m; k++) if (l[k] > u[k]) return MI_OSQP_ERR_INVALID_DATA;
  if ((rc = sync_rho_to_host(h))) return rc;
  h->host_bounds_stale = false;   // host copy becomes authoritative
  std::vector<int> changed;
  for (int q = 0; q < B; q++) {
    QPNumeric &Q = h->qp[q];
    for (int i = 0; i < m; i++) {
      Q.l[i] = std::max(l[(size_t)q * m + i], -kInfty); Q.u[i] = std::min(u[(size_t)q * m + i], kInfty);
      if (h->st.scaling) { Q.l[i] *= Q.E[i]; Q.u[i] *= Q.E[i]; }
    }
    if (refresh_rho_types(an, Q)) changed.push_back(q);
  }
  std::vector<int> all(B);
  for (int i = 0; i < B; i++) all[i] = i;
  if ((rc = upload_problem(h, all, false))) return rc;
  if ((rc = refactor_qps(h, changed))) return rc;      // constraint types changed: new rho vector + factor on the device
  if (!changed.empty() && (rc = snapshot(h))) return rc;
  return MI_OSQP_OK;
}

int mi_osqp_batch_update_bounds_device(mi_osqp_batch *h, const double *d_l, const double *d_u, void *stream) {
  if (!h || !d_l || !d_u) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  return update_bounds_on_device(h, d_l, d_u, stream ? (hipStream_t)stream : h->stream, nullptr, nullptr);
}

// (h_l / h_u: the same bounds on the host when the caller has them, else they are fetched if the host path is needed)
static int update_bounds_on_device(mi_osqp_batch *h, const double *d_l, const double *d_u, hipStream_t s, const double *h_l, const double *h_u) {
  h->clear_rho_updates = true;
  int m = (*h->anp).m, B = h->B;
  if (!m) return MI_OSQP_OK;
  // pass 1: validate + detect constraint-type changes without writing
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), s));
  HIPCHK(launch_bounds(d_l, d_u, h->out1.p /*scratch*/, h->out2.p /*scratch*/, h->Esc.p, h->rho_vec.p, h->dscal.p, h->flag.p, B,
                       m, h->BT, h->st.scaling ? 1 : 0, s));
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (flag & 2) return MI_OSQP_ERR_INVALID_DATA;
  if (flag & 1) {   // a row changed type -> needs the refactor path: go through the host
    if (h_l && h_u) return update_bounds_on_host(h, h_l, h_u);
    std::vector<double> hl((size_t)B * m), hu((size_t)B * m);
    HIPCHK(hipMemcpy(hl.data(), d_l, hl.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hu.data(), d_u, hu.size() * sizeof(double), hipMemcpyDeviceToHost));
    return update_bounds_on_host(h, hl.data(), hu.data());
  }
  HIPCHK(launch_bounds(d_l, d_u, h->l.p, h->u.p, h->Esc.p, h->rho_vec.p, h->dscal.p, h->flag.p, B, m, h->BT,
                       h->st.scaling ? 1 : 0, s));
  HIPCHK(hipStreamSynchronize(s));
  h->host_bounds_stale = true;
  return MI_OSQP_OK;
}

static int update_A_values(mi_osqp_batch *h, const int64_t *Ap, const int64_t *Ai, const double *Av);

// The host mirrors of the scaled problem after the device has re-equilibrated: fetched when a host path needs them
// (a bounds update that changes row types, MI_OSQP_HOST_RUIZ).
static int ensure_mirrors(mi_osqp_batch *h) {
  if (!h->host_scaling_stale) return 0;
  const Analysis &an = (*h->anp);
  const int n = an.n, m = an.m, B = h->B, nnzP = an.Pp[n], nnzA = an.Ap[n], pa_len = nnzP + nnzA;
  int rc;
  if ((rc = ensure_stage(h, (size_t)B * std::max({pa_len, n, m, 1}) + 1, 0))) return rc;
  std::vector<double> tmp;
  auto down = [&](const double *src, int len) -> int {
    tmp.resize((size_t)B * len);
    if (!len) return 0;
    HIPCHK(launch_deinterleave(src, h->stage.p, B, len, h->BT, h->stream));
    HIPCHK(hipMemcpyAsync(tmp.data(), h->stage.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  };
  if ((rc = down(h->pa_val.p, pa_len))) return rc;
  for (int q = 0; q < B; q++) {
    std::copy(tmp.begin() + (size_t)q * pa_len, tmp.begin() + (size_t)q * pa_len + nnzP, h->qp[q].Pv.begin());
    std::copy(tmp.begin() + (size_t)q * pa_len + nnzP, tmp.begin() + (size_t)(q + 1) * pa_len, h->qp[q].Av.begin());
  }
  if ((rc = down(h->q.p, n))) return rc;
  for (int q = 0; q < B; q++) std::copy(tmp.begin() + (size_t)q * n, tmp.begin() + (size_t)(q + 1) * n, h->qp[q].q.begin());
  if ((rc = down(h->Dsc.p, n))) return rc;
  for (int q = 0; q < B; q++) for (int j = 0; j < n; j++) { h->qp[q].D[j] = tmp[(size_t)q * n + j]; h->qp[q].Dinv[j] = 1.0 / h->qp[q].D[j]; }
  if ((rc = down(h->Esc.p, m))) return rc;
  for (int q = 0; q < B; q++) for (int i = 0; i < m; i++) { h->qp[q].E[i] = tmp[(size_t)q * m + i]; h->qp[q].Einv[i] = 1.0 / h->qp[q].E[i]; }
  const size_t dcnt = (size_t)h->ntiles * DS_COUNT * h->BT;
  HIPCHK(hipMemcpy(h->h_dscal, h->dscal.p, dcnt * sizeof(double), hipMemcpyDeviceToHost));
  for (int q = 0; q < B; q++) {
    h->qp[q].c = h->h_dscal[(size_t)(q / h->BT) * DS_COUNT * h->BT + DS_C * h->BT + q % h->BT];
    h->qp[q].cinv = 1.0 / h->qp[q].c;
  }
  h->host_scaling_stale = false;
  h->host_bounds_stale = true;
  if ((rc = sync_bounds_to_host(h))) return rc;
  for (int q = 0; q < B; q++) (void)refresh_rho_types(an, h->qp[q]);
  h->host_rho_stale = true;
  return sync_rho_to_host(h);
}

// Row E13's A / bounds update with row E2 on the device: raw values through pinned memory, ruiz_kernel (unscale, new A,
// equilibrate, scale the bounds), the check streams re-scattered, ONE refactorisation of every QP.  l / u null: bounds kept.
static int device_update(mi_osqp_batch *h, const double *Av, const double *l, const double *u,
                         const double *dA = nullptr, const double *dl = nullptr, const double *du = nullptr) {      // (dA / dl / du: the same data already in HBM)
  const Analysis &an = (*h->anp);
  const int n = an.n, m = an.m, B = h->B, nnzP = an.Pp[n], nnzA = an.Ap[n], pa_len = nnzP + nnzA;
  h->clear_rho_updates = true;
  const size_t cA = (size_t)B * nnzA, cb = (l || dl) ? (size_t)B * m : 0, cpa = (size_t)B * pa_len;
  int rc;
  if ((rc = ensure_pin(h, cA + 2 * cb + 1)) || (rc = ensure_stage(h, cA + 2 * cb + cpa + 1, (size_t)B))) return rc;
  if (!dA) {
    // through pinned memory in slices of 4 MB: the transfer of a slice runs while the host threads copy the next one
    // (256 GOMP QPs of config 4: 30 MB, ~2 ms when copied whole and then sent)
    const size_t slice = (size_t)1 << 19;
    struct Part { const double *src; size_t off, len; };
    std::vector<Part> parts{{Av, 0, cA}};
    if (l) { parts.push_back({l, cA, cb}); parts.push_back({u, cA + cb, cb}); }
    for (const Part &pt : parts)
      for (size_t o = 0; o < pt.len; o += slice) {
        const size_t len = std::min(slice, pt.len - o);
        par_copy(h->pin + pt.off + o, pt.src + o, len);
        HIPCHK(hipMemcpyAsync(h->stage.p + pt.off + o, h->pin + pt.off + o, len * sizeof(double), hipMemcpyHostToDevice, h->stream));
      }
  }
  RuizArgs r{};
  r.n = n; r.m = m; r.nnzP = nnzP; r.nnzA = nnzA; r.B = B; r.BT = h->BT; r.iters = (int)h->st.scaling;
  r.Prow = h->rz_prow.p; r.Pcol = h->rz_pcol.p; r.Arow = h->rz_arow.p; r.Acol = h->rz_acol.p;
  if (dA) { r.rawA = dA; r.rawl = dl; r.rawu = du; }
  else { r.rawA = h->stage.p; r.rawl = l ? h->stage.p + cA : nullptr; r.rawu = l ? h->stage.p + cA + cb : nullptr; }
  r.pa_val = h->pa_val.p; r.q = h->q.p; r.Dsc = h->Dsc.p; r.Dsc_inv = h->Dsc_inv.p; r.Esc = h->Esc.p; r.Esc_inv = h->Esc_inv.p;
  r.l = h->l.p; r.u = h->u.p; r.dscal = h->dscal.p;
  r.dn = h->out1.p; r.en = h->out1.p + (size_t)B * n;              // (scratch of check_kernel: (2n + m) doubles per QP)
  r.pa_out = h->stage.p + cA + 2 * cb;
  HIPCHK(launch_ruiz(r, h->stream));
  std::vector<int> ids(B);
  for (int i = 0; i < B; i++) ids[i] = i;
  HIPCHK(hipMemcpyAsync(h->ids.p, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(launch_scatter(r.pa_out, h->chk_val.p, h->chk.src.p, h->ids.p, B, pa_len, h->chk.view(an.chk), h->BT, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->host_scaling_stale = true; h->host_bounds_stale = true; h->host_rho_stale = true;
  if ((rc = refactor_qps(h, std::move(ids)))) return rc;          // (factor_kernel derives the rho vectors from the bounds in force)
  return snapshot(h);
}
// Device or host equilibration: ruiz_kernel gives every QP one workgroup - right for a batch (256 GOMP QPs: 22 -> 7 ms per
// update), wrong for a handful of large QPs (one QP of 48 k entries: 5 ms on a host thread, 14 ms in one workgroup).
// MI_OSQP_HOST_RUIZ=1 / MI_OSQP_DEVICE_RUIZ=1 force one or the other (same bits either way).
static bool host_ruiz(const mi_osqp_batch *h) {
  if (h->tune.ruiz) return h->tune.ruiz > 0;
  const Analysis &an = (*h->anp);
  const long per_qp = (long)an.Pp[an.n] + an.Ap[an.n] + an.n + an.m;
  return h->B < 16 || per_qp > 65536;
}

int mi_osqp_batch_update_A(mi_osqp_batch *h, const int64_t *Ap, const int64_t *Ai, const double *Av) {
  CallTimer timer_("batch_update_A");
  if (!h || !Ap || !Ai || !Av) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const Analysis &an = (*h->anp);
  for (int j = 0; j <= an.n; j++) if (Ap[j] != an.Ap[j]) return MI_OSQP_ERR_PATTERN_CHANGED;
  for (int k = 0; k < an.Ap[an.n]; k++) if (Ai[k] != an.Ai[k]) return MI_OSQP_ERR_PATTERN_CHANGED;
  if (!host_ruiz(h)) return device_update(h, Av, nullptr, nullptr);
  int rc = update_A_values(h, Ap, Ai, Av);
  if (rc || (rc = mi_osqp_batch_refactor_device(h))) return rc;
  return snapshot(h);
}

// QPSolver::update with the new values already in HBM (QP-major [B][nnzA], [B][m], natural CSC order of the pattern given at
// setup - a planner that assembles its rows on the device, or mi_gomp_scene): nothing crosses PCIe but a validation flag.
int mi_osqp_batch_update_A_bounds_device(mi_osqp_batch *h, const double *d_Av, const double *d_l, const double *d_u, void *stream) {
  CallTimer timer_("batch_update_A_bounds_device");
  if (!h || !d_Av || !d_l || !d_u) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const Analysis &an = (*h->anp);
  const int m = an.m, B = h->B, nnzA = an.Ap[an.n];
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (host_ruiz(h)) {            // a handful of large QPs: equilibrated on host threads, so the values come down first
    std::vector<double> hA((size_t)B * nnzA), hl((size_t)B * m), hu((size_t)B * m);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(hA.data(), d_Av, hA.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hl.data(), d_l, hl.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hu.data(), d_u, hu.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int64_t> Ap(an.Ap.begin(), an.Ap.end()), Ai(an.Ai.begin(), an.Ai.end());
    return mi_osqp_batch_update_A_bounds(h, Ap.data(), Ai.data(), hA.data(), hl.data(), hu.data());
  }
  if (m) {                       // l <= u, checked without writing (pass 1 of the bounds update)
    HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), s));
    HIPCHK(launch_bounds(d_l, d_u, h->out1.p, h->out2.p, h->Esc.p, h->rho_vec.p, h->dscal.p, h->flag.p, B, m, h->BT, h->st.scaling ? 1 : 0, s));
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flag & 2) return MI_OSQP_ERR_INVALID_DATA;
  } else HIPCHK(hipStreamSynchronize(s));
  return device_update(h, nullptr, nullptr, nullptr, d_Av, d_l, d_u);
}

// new A values and new bounds, ONE refactorisation (QPSolver::update: [REF] src/osqp-wrapper.h:33-43)
int mi_osqp_batch_update_A_bounds(mi_osqp_batch *h, const int64_t *Ap, const int64_t *Ai, const double *Av, const double *l, const double *u) {
  CallTimer timer_("batch_update_A_bounds");
  if (!h || !Ap || !Ai || !Av || !l || !u) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const Analysis &an = (*h->anp);
  const int m = an.m, B = h->B;
  {
    const size_t tot = (size_t)B * m, chunk = (size_t)1 << 17;
    std::atomic<int> bad{0};
    const int parts = (int)((tot + chunk - 1) / chunk);
    auto scan = [&](int i, int) { const size_t e = std::min(tot, ((size_t)i + 1) * chunk); for (size_t k = (size_t)i * chunk; k < e; k++) if (l[k] > u[k]) { bad.store(1); return; } };
    if (parts <= 2) { for (int i = 0; i < parts; i++) scan(i, 0); } else parallel_for(parts, scan);
    if (bad.load()) return MI_OSQP_ERR_INVALID_DATA;
  }
  for (int j = 0; j <= an.n; j++) if (Ap[j] != an.Ap[j]) return MI_OSQP_ERR_PATTERN_CHANGED;
  for (int k = 0; k < an.Ap[an.n]; k++) if (Ai[k] != an.Ai[k]) return MI_OSQP_ERR_PATTERN_CHANGED;
  if (!host_ruiz(h)) return device_update(h, Av, l, u);
  int rc = update_A_values(h, Ap, Ai, Av);        // (the host mirrors are authoritative from here on)
  if (rc) return rc;
  for (int q = 0; q < B; q++) {
    QPNumeric &Q = h->qp[q];
    for (int i = 0; i < m; i++) {
      Q.l[i] = std::max(l[(size_t)q * m + i], -kInfty); Q.u[i] = std::min(u[(size_t)q * m + i], kInfty);
      if (h->st.scaling) { Q.l[i] *= Q.E[i]; Q.u[i] *= Q.E[i]; }
    }
    (void)refresh_rho_types(an, Q);
  }
  std::vector<int> all(B);
  for (int i = 0; i < B; i++) all[i] = i;
  if ((rc = upload_problem(h, all, false)) || (rc = refactor_qps(h, all))) return rc;       // (factor_kernel derives the rho vectors from the new bounds)
  return snapshot(h);
}

static int update_A_values(mi_osqp_batch *h, const int64_t *Ap, const int64_t *Ai, const double *Av) {
  { int rc0 = ensure_mirrors(h); if (rc0) return rc0; }
  h->clear_rho_updates = true;
  const Analysis &an = (*h->anp);
  int n = an.n, B = h->B, nnzA = an.Ap[n], rc;
  for (int j = 0; j <= n; j++) if (Ap[j] != an.Ap[j]) return MI_OSQP_ERR_PATTERN_CHANGED;
  for (int k = 0; k < nnzA; k++) if (Ai[k] != an.Ai[k]) return MI_OSQP_ERR_PATTERN_CHANGED;
  if ((rc = sync_bounds_to_host(h)) || (rc = sync_rho_to_host(h))) return rc;
  // host: unscale, new values, Ruiz rescale (O(nnz) per QP); device: the numeric refactorisation of every QP
  // (factor_kernel on the new scaled values and the current rho vectors) - the same code path a rho update takes
  const int CH = 128;
  for (int c0 = 0; c0 < B; c0 += CH) {
    int c1 = std::min(B, c0 + CH);
    parallel_for(c1 - c0, [&](int k, int) {
      int qi = c0 + k;
      QPNumeric &Q = h->qp[qi];
      if (h->st.scaling) unscale_qp(an, Q);
      std::copy(Av + (size_t)qi * nnzA, Av + (size_t)(qi + 1) * nnzA, Q.Av.begin());
      if (h->st.scaling) scale_qp(an, h->st, Q);
    });
    std::vector<int> ids(c1 - c0);
    for (int k = 0; k < c1 - c0; k++) ids[k] = c0 + k;
    if ((rc = upload_problem(h, ids, true)) || (rc = sync_scalars_to_device(h, ids, true))) return rc;
  }
  return MI_OSQP_OK;
}

int mi_osqp_batch_refactor_device(mi_osqp_batch *h) {
  if (!h) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  std::vector<int> all(h->B);
  for (int i = 0; i < h->B; i++) all[i] = i;
  return refactor_qps(h, std::move(all));
}

// ------------------------------------------------------------------ objective updates
// osqp_update_lin_cost / osqp_update_P / osqp_update_P_A / osqp_warm_start_y (OSQP 0.6.x semantics, README "Objective updates").

// triu(P) of a P given in the form setup accepts (both triangles or the upper one), extracted as analyze() does: src[t] =
// position in the caller's value array of the t-th entry of the analysis's triu(P).  false: the pattern differs.
static bool triu_sources(const Analysis &an, const int64_t *Pp, const int64_t *Pi, std::vector<int64_t> &src) {
  const int n = an.n;
  src.clear();
  src.reserve((size_t)an.Pp[n]);
  if (Pp[0] != 0) return false;
  for (int j = 0; j < n; j++) {
    for (int64_t k = Pp[j]; k < Pp[j + 1]; k++)
      if (Pi[k] <= j) {
        const size_t t = src.size();
        if ((int64_t)t >= an.Pp[j + 1] || Pi[k] != an.Pi[t]) return false;
        src.push_back(k);
      }
    if ((int64_t)src.size() != an.Pp[j + 1]) return false;
  }
  return true;
}
static bool same_A_pattern(const Analysis &an, const int64_t *Ap, const int64_t *Ai) {
  for (int j = 0; j <= an.n; j++) if (Ap[j] != an.Ap[j]) return false;
  for (int k = 0; k < an.Ap[an.n]; k++) if (Ai[k] != an.Ai[k]) return false;
  return true;
}

// q -> h->q (scaled with the D and c in force) and rawq, on `s`; the host mirrors follow (q_host) or are marked stale
static int update_q_impl(mi_osqp_batch *h, const double *q_host, const double *d_q, hipStream_t s) {
  const Analysis &an = (*h->anp);
  const int n = an.n, B = h->B;
  const size_t cnt = (size_t)B * n;
  h->clear_rho_updates = true;
  int rc;
  if (q_host) {
    if ((rc = ensure_stage(h, cnt, 0)) || (rc = ensure_pin(h, cnt))) return rc;
    const size_t slice = (size_t)1 << 19;          // 4 MB slices, as mi_osqp_batch_update_bounds
    for (size_t o = 0; o < cnt; o += slice) {
      const size_t len = std::min(slice, cnt - o);
      par_copy(h->pin + o, q_host + o, len);
      HIPCHK(hipMemcpyAsync(h->stage.p + o, h->pin + o, len * sizeof(double), hipMemcpyHostToDevice, s));
    }
    d_q = h->stage.p;
  }
  HIPCHK(launch_lin_cost(d_q, nullptr, h->q.p, h->rawq.p, h->Dsc.p, h->dscal.p, B, n, h->BT, h->st.scaling ? 1 : 0, s));
  HIPCHK(hipStreamSynchronize(s));
  if (h->host_scaling_stale) return MI_OSQP_OK;       // (the mirrors are fetched whole when a host path needs them)
  if (!q_host) { h->host_scaling_stale = true; return MI_OSQP_OK; }
  parallel_for(B, [&](int qi, int) {
    QPNumeric &Q = h->qp[qi];
    for (int j = 0; j < n; j++) {
      double v = q_host[(size_t)qi * n + j];
      if (h->st.scaling) { v *= Q.D[j]; v *= Q.c; }
      Q.q[j] = v;
    }
  });
  return MI_OSQP_OK;
}

// New values of triu(P) (and of A when Av != null): unscale with the scaling in force, replace, equilibrate again from
// P, q and A, rescale the bounds, refactor every QP with its current rho vectors, snapshot - as mi_osqp_batch_update_A
// does for A.  src: triu_sources() of the caller's P (null: Pv is triu(P) in the analysis's order already).
// dP (and dA, dl, du - all three or none): the same data in HBM, [B][nnzP] in the analysis's order, [B][nnzA], [B][m]; only
// handles that equilibrate on the device take them.  l, u: new bounds on the host, for handles that equilibrate there.
static int update_P_impl(mi_osqp_batch *h, const std::vector<int64_t> *src, int64_t nnzPin, const double *Pv, const double *Av,
                         const double *l = nullptr, const double *u = nullptr,
                         const double *dP = nullptr, const double *dA = nullptr, const double *dl = nullptr, const double *du = nullptr) {
  const Analysis &an = (*h->anp);
  const int n = an.n, m = an.m, B = h->B, nnzP = an.Pp[n], nnzA = an.Ap[n], pa_len = nnzP + nnzA;
  h->clear_rho_updates = true;
  int rc;
  const size_t cP = dP ? 0 : (size_t)B * nnzP, cA = Av ? (size_t)B * nnzA : 0, cpa = (size_t)B * pa_len;      // (what is staged)
  if ((rc = ensure_pin(h, cP + cA + 1)) || (rc = ensure_stage(h, cP + cA + cpa + 1, (size_t)B))) return rc;
  if (dP) {
    if ((size_t)B * nnzP) HIPCHK(hipMemcpyAsync(h->rawP.p, dP, (size_t)B * nnzP * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  } else {
    // the new triu(P) of every QP, QP-major in the analysis's order (what rawP keeps)
    parallel_for(B, [&](int qi, int) {
      double *dst = h->pin + (size_t)qi * nnzP;
      const double *sv = Pv + (size_t)qi * nnzPin;
      for (int t = 0; t < nnzP; t++) dst[t] = sv[src ? (*src)[t] : t];
    });
    if (Av) par_copy(h->pin + cP, Av, cA);
    if (cP + cA) HIPCHK(hipMemcpyAsync(h->stage.p, h->pin, (cP + cA) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (cP) HIPCHK(hipMemcpyAsync(h->rawP.p, h->stage.p, cP * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  }
  std::vector<int> all(B);
  for (int i = 0; i < B; i++) all[i] = i;
  if (!host_ruiz(h)) {
    RuizArgs r{};
    r.n = n; r.m = m; r.nnzP = nnzP; r.nnzA = nnzA; r.B = B; r.BT = h->BT; r.iters = (int)h->st.scaling;
    r.Prow = h->rz_prow.p; r.Pcol = h->rz_pcol.p; r.Arow = h->rz_arow.p; r.Acol = h->rz_acol.p;
    if (dP) { r.rawPnew = dP; r.rawA = dA; r.rawl = dl; r.rawu = du; }
    else { r.rawPnew = h->stage.p; r.rawA = Av ? h->stage.p + cP : nullptr; r.rawl = r.rawu = nullptr; }
    r.pa_val = h->pa_val.p; r.q = h->q.p; r.Dsc = h->Dsc.p; r.Dsc_inv = h->Dsc_inv.p; r.Esc = h->Esc.p; r.Esc_inv = h->Esc_inv.p;
    r.l = h->l.p; r.u = h->u.p; r.dscal = h->dscal.p;
    r.dn = h->out1.p; r.en = h->out1.p + (size_t)B * n;              // (scratch of check_kernel: (2n + m) doubles per QP)
    r.pa_out = h->stage.p + cP + cA;
    HIPCHK(launch_ruiz(r, h->stream));
    HIPCHK(hipMemcpyAsync(h->ids.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(launch_scatter(r.pa_out, h->chk_val.p, h->chk.src.p, h->ids.p, B, pa_len, h->chk.view(an.chk), h->BT, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->host_scaling_stale = true; h->host_bounds_stale = true; h->host_rho_stale = true;
  } else {
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((rc = ensure_mirrors(h)) || (rc = sync_bounds_to_host(h)) || (rc = sync_rho_to_host(h))) return rc;
    const int CH = 128;
    for (int c0 = 0; c0 < B; c0 += CH) {
      const int c1 = std::min(B, c0 + CH);
      parallel_for(c1 - c0, [&](int k, int) {
        const int qi = c0 + k;
        QPNumeric &Q = h->qp[qi];
        if (h->st.scaling) unscale_qp(an, Q);
        const double *sv = Pv + (size_t)qi * nnzPin;
        for (int t = 0; t < nnzP; t++) Q.Pv[t] = sv[src ? (*src)[t] : t];
        if (Av) std::copy(Av + (size_t)qi * nnzA, Av + (size_t)(qi + 1) * nnzA, Q.Av.begin());
        if (h->st.scaling) scale_qp(an, h->st, Q);
        if (l) {          // (as mi_osqp_batch_update_A_bounds: the new bounds under the new E)
          for (int i = 0; i < m; i++) {
            Q.l[i] = std::max(l[(size_t)qi * m + i], -kInfty); Q.u[i] = std::min(u[(size_t)qi * m + i], kInfty);
            if (h->st.scaling) { Q.l[i] *= Q.E[i]; Q.u[i] *= Q.E[i]; }
          }
          (void)refresh_rho_types(an, Q);
        }
      });
      std::vector<int> ids(all.begin() + c0, all.begin() + c1);
      if ((rc = upload_problem(h, ids, true)) || (rc = sync_scalars_to_device(h, ids, true))) return rc;
    }
  }
  if ((rc = refactor_qps(h, std::move(all)))) return rc;          // (the rho vectors in force; factor_kernel re-derives them from the bounds)
  return snapshot(h);
}

static int update_P_checked(mi_osqp_batch *h, const int64_t *Pp, const int64_t *Pi, const double *Pv,
                            const int64_t *Ap, const int64_t *Ai, const double *Av) {
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const Analysis &an = (*h->anp);
  std::vector<int64_t> src;
  if (!triu_sources(an, Pp, Pi, src)) return MI_OSQP_ERR_PATTERN_CHANGED;
  if (Av && !same_A_pattern(an, Ap, Ai)) return MI_OSQP_ERR_PATTERN_CHANGED;
  return update_P_impl(h, &src, Pp[an.n], Pv, Av);
}

int mi_osqp_batch_update_q(mi_osqp_batch *h, const double *q) {
  CallTimer timer_("batch_update_q");
  if (!h || !q) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  return update_q_impl(h, q, nullptr, h->stream);
}

int mi_osqp_batch_update_q_device(mi_osqp_batch *h, const double *d_q, void *stream) {
  CallTimer timer_("batch_update_q_device");
  if (!h || !d_q) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  return update_q_impl(h, nullptr, d_q, stream ? (hipStream_t)stream : h->stream);
}

int mi_osqp_batch_update_P(mi_osqp_batch *h, const int64_t *Pp, const int64_t *Pi, const double *Pv) {
  CallTimer timer_("batch_update_P");
  if (!h || !Pp || !Pi || !Pv) return MI_OSQP_ERR_NULL;
  return update_P_checked(h, Pp, Pi, Pv, nullptr, nullptr, nullptr);
}

int mi_osqp_batch_update_P_A(mi_osqp_batch *h, const int64_t *Pp, const int64_t *Pi, const double *Pv,
                             const int64_t *Ap, const int64_t *Ai, const double *Av) {
  CallTimer timer_("batch_update_P_A");
  if (!h || !Pp || !Pi || !Pv || !Ap || !Ai || !Av) return MI_OSQP_ERR_NULL;
  return update_P_checked(h, Pp, Pi, Pv, Ap, Ai, Av);
}

int mi_osqp_batch_get_P_upper_pattern(mi_osqp_batch *h, int64_t *colptr, int64_t *rowidx, int64_t *nnz_out) {
  if (!h || !nnz_out) return MI_OSQP_ERR_NULL;
  const Analysis &an = (*h->anp);
  *nnz_out = an.Pp[an.n];
  if (colptr) for (int j = 0; j <= an.n; j++) colptr[j] = an.Pp[j];
  if (rowidx) for (int k = 0; k < an.Pp[an.n]; k++) rowidx[k] = an.Pi[k];
  return MI_OSQP_OK;
}

// osqp_update_P (+ QPSolver::update) with the new values in HBM: triu(P) [B][nnzPu] in the analysis's order - the layout of
// the adjoint's dP - and optionally A [B][nnzA] and the bounds [B][m].  One equilibration, one refactorisation, one snapshot.
static int update_P_device_impl(mi_osqp_batch *h, const double *d_Pv, const double *d_Av, const double *d_l, const double *d_u, hipStream_t s) {
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  const Analysis &an = (*h->anp);
  const int m = an.m, B = h->B, nnzP = an.Pp[an.n], nnzA = an.Ap[an.n];
  if (host_ruiz(h)) {            // equilibrated on host threads, so the values come down first (as mi_osqp_batch_update_A_bounds_device)
    std::vector<double> hP((size_t)B * nnzP), hA, hl, hu;
    HIPCHK(hipStreamSynchronize(s));
    if (!hP.empty()) HIPCHK(hipMemcpy(hP.data(), d_Pv, hP.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (d_Av) {
      hA.resize((size_t)B * nnzA); hl.resize((size_t)B * m); hu.resize((size_t)B * m);
      if (!hA.empty()) HIPCHK(hipMemcpy(hA.data(), d_Av, hA.size() * sizeof(double), hipMemcpyDeviceToHost));
      if (m) {
        HIPCHK(hipMemcpy(hl.data(), d_l, hl.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hu.data(), d_u, hu.size() * sizeof(double), hipMemcpyDeviceToHost));
      }
      for (size_t k = 0; k < hl.size(); k++) if (hl[k] > hu[k]) return MI_OSQP_ERR_INVALID_DATA;
    }
    return update_P_impl(h, nullptr, nnzP, hP.data(), d_Av ? hA.data() : nullptr, d_Av ? hl.data() : nullptr, d_Av ? hu.data() : nullptr);
  }
  if (d_Av && m) {               // l <= u, checked without writing (pass 1 of the bounds update)
    HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), s));
    HIPCHK(launch_bounds(d_l, d_u, h->out1.p, h->out2.p, h->Esc.p, h->rho_vec.p, h->dscal.p, h->flag.p, B, m, h->BT, h->st.scaling ? 1 : 0, s));
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flag & 2) return MI_OSQP_ERR_INVALID_DATA;
  } else HIPCHK(hipStreamSynchronize(s));
  return update_P_impl(h, nullptr, nnzP, nullptr, nullptr, nullptr, nullptr, d_Pv, d_Av, d_l, d_u);
}

int mi_osqp_batch_update_P_device(mi_osqp_batch *h, const double *d_Pv, void *stream) {
  CallTimer timer_("batch_update_P_device");
  if (!h || !d_Pv) return MI_OSQP_ERR_NULL;
  return update_P_device_impl(h, d_Pv, nullptr, nullptr, nullptr, stream ? (hipStream_t)stream : h->stream);
}

int mi_osqp_batch_update_P_A_bounds_device(mi_osqp_batch *h, const double *d_Pv, const double *d_Av, const double *d_l, const double *d_u,
                                           void *stream) {
  if (!h) return MI_OSQP_ERR_NULL;
  const int given = (d_Av ? 1 : 0) + (d_l ? 1 : 0) + (d_u ? 1 : 0);
  if (given != 0 && given != 3) return MI_OSQP_ERR_NULL;           // (A and the bounds come together or not at all)
  if (!d_Pv) return given ? mi_osqp_batch_update_A_bounds_device(h, d_Av, d_l, d_u, stream) : MI_OSQP_ERR_NULL;
  if (!given) return mi_osqp_batch_update_P_device(h, d_Pv, stream);
  CallTimer timer_("batch_update_P_A_bounds_device");
  return update_P_device_impl(h, d_Pv, d_Av, d_l, d_u, stream ? (hipStream_t)stream : h->stream);
}

int mi_osqp_batch_warm_start_y(mi_osqp_batch *h, const double *y) {
  CallTimer timer_("batch_warm_start_y");
  if (!h || !y) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  { const int rc_ = cont_leave(h); if (rc_) return rc_; }
  h->st.warm_start = 1;
  const size_t cnt = (size_t)h->B * (*h->anp).m;
  if (!cnt) return MI_OSQP_OK;
  int rc;
  if ((rc = ensure_stage(h, cnt, 0)) || (rc = ensure_pin(h, cnt))) return rc;
  par_copy(h->pin, y, cnt);
  HIPCHK(hipMemcpyAsync(h->stage.p, h->pin, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KernelArgs a = make_args(h);
  HIPCHK(launch_warm_start_y(a, h->ntiles * h->BT, h->BT, h->stream, h->stage.p));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MI_OSQP_OK;
}

int mi_osqp_batch_spmv(mi_osqp_batch *h, const double *d_x, const double *d_y, double *d_Px, double *d_Aty, double *d_Ax,
                       void *stream) {
  if (!h) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  KernelArgs a = make_args(h);
  if (h->sp_ptr.n) {      // one read of P and A for all three products
    SpmvFused t{};
    t.ptr = h->sp_ptr.p; t.ent = h->sp_ent.p; t.pa_val = h->pa_val.p; t.pa_len = (*h->anp).Pp[(*h->anp).n] + (*h->anp).Ap[(*h->anp).n];
    if (h->sp_npass) {
      t.ell = h->sp_ell.p; t.rowid = h->sp_rowid.p; t.n_pass = h->sp_npass;
      for (int p = 0; p < 4; p++) { t.ell_off[p] = h->sp_ell_off[p]; t.ell_k[p] = h->sp_ell_k[p]; }
    }
    HIPCHK(launch_spmv_fused(a, t, h->BT, h->ntiles, h->n_cus, s, d_x, d_y, d_Px, d_Aty, d_Ax));
    HIPCHK(hipStreamSynchronize(s));
    return MI_OSQP_OK;
  }
  size_t lds = (size_t)((*h->anp).Next + 2 * (*h->anp).n + (*h->anp).m) * h->BT * sizeof(double);
  a.op_out_lds = !h->global_xs && lds <= 160 * 1024 - 1024;
  if (!a.op_out_lds) lds = h->lds;
  HIPCHK(launch_spmv(a, h->BT, h->ntiles, h->threads, lds, s, d_x, d_y, d_Px, d_Aty, d_Ax));
  HIPCHK(hipStreamSynchronize(s));
  return MI_OSQP_OK;
}

int mi_osqp_batch_kkt_solve(mi_osqp_batch *h, const double *d_rhs, double *d_sol, void *stream) {
  if (!h || !d_rhs || !d_sol) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  KernelArgs a = make_args(h);
  return run_spinning(h, s, [&]() -> int {
    HIPCHK(launch_kkt_solve(a, h->BT, h->ntiles, h->mw_groups > 0 ? h->mw_threads : h->threads, h->lds, s, d_rhs, d_sol));
    return MI_OSQP_OK;
  });
}

int mi_osqp_debug_trace_kkt_solve(mi_osqp_batch *h, int32_t which, const double *d_rhs, double *d_sol, uint32_t *out,
                                  int64_t cap, int64_t *dims) {
  if (!h || !dims) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  const int nw = h->threads / 64;
  const int64_t fp = (*h->anp).fwd.n_phases, bp = (*h->anp).bwd.n_phases, words = 8 + 4 * nw + (fp + bp) * nw * 2;
  dims[0] = fp; dims[1] = bp; dims[2] = nw; dims[3] = words;
  if (!out) return MI_OSQP_OK;
  if (which == 1 || which == 2) {
    const Schedule &sc = which == 1 ? (*h->anp).fwd : (*h->anp).bwd;
    if ((int64_t)sc.phase.size() > cap) { g_last_error = "trace: output too small"; return MI_OSQP_ERR_INVALID_DATA; }
    std::copy(sc.phase.begin(), sc.phase.end(), out);
    return MI_OSQP_OK;
  }
  if (!d_rhs || !d_sol) return MI_OSQP_ERR_NULL;
  if (2 * words > cap) { g_last_error = "trace: output too small"; return MI_OSQP_ERR_INVALID_DATA; }
  uint32_t *d_tr = nullptr;
  HIPCHK(hipMalloc(&d_tr, (size_t)2 * words * 4));
  KernelArgs a = make_args(h);
  hipError_t e = launch_kkt_trace(a, h->BT, h->ntiles, h->threads, h->lds, h->stream, d_rhs, d_sol, d_tr, (uint32_t)words);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_tr, (size_t)2 * words * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d_tr);
  HIPCHK(e);
  return MI_OSQP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ continuous
// Per-QP entry points + a non-blocking advance: the reference's SQP loop is per trajectory - solve, check, re-linearise,
// update, solve again ([REF] src/gomp-solver.h:70-88) - so the QPs of a batch do not finish together and must not wait
// for each other.  A QP's solve is begun with solve_begin_some, advance() enqueues one segment (L iterations + check +
// the refactorisations the check asks for) for every QP that is iterating, poll() reports the QPs that finished, and the
// caller updates / warm-starts / begins them again while the rest keeps iterating.  Every QP counts its iterations from
// its own begin (IS_CUR), so it takes exactly the iterations, rho updates and checks of a blocking solve of its own:
// results are those of mi_osqp_batch_solve bit for bit.  Nothing in these calls waits for the device except poll().

static int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// iterations per segment of advance_kernel: the gcd of the periods at which a solve looks at itself
static int segment_length(const Settings &S) {
  int L = (int)S.max_iter;
  if (S.check_termination > 0) L = gcd_i(L, (int)S.check_termination);
  if (S.adaptive_rho && S.adaptive_rho_interval > 0) L = gcd_i(L, (int)S.adaptive_rho_interval);
  return std::max(1, L);
}
// the pinned images advance_kernel publishes flags / scalars in, its tile counter and completion word
static int ensure_advance_buffers(mi_osqp_batch *h) {
  mi_osqp_batch::Cont &c = h->cont;
  const size_t icnt = (size_t)h->ntiles * IS_COUNT * h->BT, dcnt = (size_t)h->ntiles * DS_COUNT * h->BT;
  for (int k = 0; k < 2; k++) {
    if (!c.h_is[k]) HIPCHK(hostpool::alloc((void **)&c.h_is[k], icnt * sizeof(int), &c.h_is_cap[k]));
    if (!c.h_ds[k]) HIPCHK(hostpool::alloc((void **)&c.h_ds[k], dcnt * sizeof(double), &c.h_ds_cap[k]));
  }
  int rc;
  if (!c.counter.p) { if ((rc = c.counter.alloc(4)) || (rc = c.counter.zero(h->stream))) return rc; }
  if (!c.h_done) { HIPCHK(hostpool::alloc((void **)&c.h_done, 64, &c.h_done_cap)); c.h_done[0] = c.h_done[1] = 0; }
  return MI_OSQP_OK;
}
// a QP of the flags in h_iscal ended its last solve with an infeasibility certificate
static bool any_cert_status(const mi_osqp_batch *h) {
  const int BT = h->BT;
  for (int q = 0; q < h->B; q++) {
    const int st = h->h_iscal[(size_t)(q / BT) * IS_COUNT * BT + IS_STATUS * BT + q % BT];
    if (st == -3 || st == 3 || st == -4 || st == 4) return true;
  }
  return false;
}
static int cont_enter(mi_osqp_batch *h) {
  mi_osqp_batch::Cont &c = h->cont;
  if (c.on) return MI_OSQP_OK;
  if (h->global_xs || h->mw_groups > 0) { g_last_error = "continuous batching serves LDS-resident QPs (a large single QP has no batch to be continuous in)"; return MI_OSQP_ERR_INVALID_DATA; }
  const Analysis &an = (*h->anp);
  const int B = h->B, n = an.n, m = an.m, BT = h->BT, nslots = h->ntiles * BT;
  c.L = segment_length(h->st);
  c.running.assign((size_t)B, 0); c.clear_rho.assign((size_t)B, 0); c.epoch.assign((size_t)B, 0);
  c.info.assign((size_t)B, mi_osqp_info{});
  c.cert_status.assign((size_t)B, 0);
  c.polishable.assign((size_t)B, 0); c.polishing.assign((size_t)B, 0);
  c.pol_status.assign((size_t)B, 0);
  if (!h->st.polish && h->pol_status.size() == (size_t)B) c.pol_status = h->pol_status;      // (an earlier continuous phase polished)
  c.n_running = 0; c.adv_seq = c.polled_seq = 0; c.launch_seq = 0;
  const size_t icnt = (size_t)h->ntiles * IS_COUNT * BT;
  { const int rc0 = ensure_advance_buffers(h); if (rc0) return rc0; }
  for (int k = 0; k < 2; k++) {
    if (!c.ev[k]) HIPCHK(hipEventCreateWithFlags(&c.ev[k], hipEventDisableTiming));
    c.seq_of[k] = 0;
  }
  if (!c.xh) HIPCHK(hostpool::alloc((void **)&c.xh, (size_t)B * n * sizeof(double), &c.xh_cap));
  if (!c.yh) HIPCHK(hostpool::alloc((void **)&c.yh, (size_t)B * std::max(m, 1) * sizeof(double), &c.yh_cap));
  const size_t cert_bytes = (size_t)B * std::max(std::max(n, m), 1) * sizeof(double);
  if (!c.ch) HIPCHK(hostpool::alloc((void **)&c.ch, cert_bytes, &c.ch_cap));
  if (!c.ring_h) {
    // a few rounds of per-QP calls: (A values + bounds + a warm start) of every QP, twice
    const size_t per_qp = ((size_t)an.Ap[n] + (size_t)an.Pp[n] + 2 * (size_t)m + (size_t)n + 16) * sizeof(double);      // (a whole call - ids, rows in, scaled values out - fits one lap)
    size_t want = std::max<size_t>((size_t)4 << 20, std::min<size_t>((size_t)256 << 20, 2 * per_qp * (size_t)B));
    // (tests: MI_OSQP_CONT_RING_KB = a ring barely larger than one whole-batch call, so that every few calls wrap)
    if (h->tune.cont_ring_kb >= 0) want = std::max<size_t>((size_t)h->tune.cont_ring_kb << 10, per_qp * (size_t)B + ((size_t)64 << 10));
    HIPCHK(hostpool::alloc((void **)&c.ring_h, want, &c.ring_h_cap));
    c.ring_cap = c.ring_h_cap;
    int rc = c.ring_d.alloc(c.ring_cap);
    if (rc) return rc;
    c.ring_head = 0;
  }
  int rc;
  if (c.work.n < (size_t)nslots + 4 && (rc = c.work.alloc((size_t)nslots + 4))) return rc;
  if (!c.ev_adv) {
    // The preparation and the refactorisations share the handle's stream with the advance launches (in order): measured on
    // the GOMP obstacle scene (ten handles driven by ten host threads) a second stream per handle LOSES - 20 streams on the
    // runtime's 4-10 hardware queues wait for each other's kernels (900 against 620 trajectories/s, profiles/r03).
    HIPCHK(hipEventCreateWithFlags(&c.ev_adv, hipEventDisableTiming));
    if ((rc = c.rz_scratch.alloc((size_t)B * (n + m) + 1))) return rc;
  }
  if ((rc = c.counter.zero(h->stream))) return rc;
  c.h_done[0] = c.h_done[1] = 0;
  // the state of the last blocking solve, if any, stays valid; every slot is idle until its solve is begun
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->h_iscal, h->iscal.p, icnt * sizeof(int), hipMemcpyDeviceToHost));
  // ... and so do its results: the pinned images start as what the whole-batch getters return now (a block of the pool
  // holds another handle's rows, and a handle's own images those of its last phase), so that a QP which finishes no solve in
  // this phase reads the same through the *_some getters and has the same rows handed back by cont_leave
  HIPCHK(hipMemcpy(c.xh, h->x_out.p, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost));
  if (m) HIPCHK(hipMemcpy(c.yh, h->y_out.p, (size_t)B * m * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(h->h_dscal, h->dscal.p, (size_t)h->ntiles * DS_COUNT * BT * sizeof(double), hipMemcpyDeviceToHost));
  // (the certificates of the last blocking solve stay with their QPs - cont_leave hands the image back; most batches have none)
  if (any_cert_status(h)) HIPCHK(hipMemcpy(c.ch, h->cert_out.p, cert_bytes, hipMemcpyDeviceToHost));
  for (int t = 0; t < h->ntiles; t++)
    for (int b = 0; b < BT; b++) {
      int *p = h->h_iscal + (size_t)t * IS_COUNT * BT;
      p[IS_DONE * BT + b] = 1; p[IS_CUR * BT + b] = 0; p[IS_PENDING * BT + b] = 0; p[IS_EPOCH * BT + b] = 0;
      if (h->clear_rho_updates) p[IS_RHO_UPDATES * BT + b] = 0;
      if (t * BT + b < B && h->failed[(size_t)t * BT + b]) p[IS_NEED_REFACTOR * BT + b] = -1;
    }
  h->clear_rho_updates = false;
  h->solved_once = true;               // (a QP never solved keeps the -10 of setup: it reads as unsolved in every getter, and the adjoint skips it)
  // get_info_some until the QP's first report of this phase: what mi_osqp_batch_get_info returns once the phase is over
  for (int q = 0; q < B; q++) info_from_images(h, q, c.info[(size_t)q]);
  HIPCHK(hipMemcpyAsync(h->iscal.p, h->h_iscal, icnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  memcpy(c.h_is[0], h->h_iscal, icnt * sizeof(int)); memcpy(c.h_is[1], h->h_iscal, icnt * sizeof(int));      // the host images advance_kernel writes
  if (!c.stop.p && (rc = c.stop.alloc(4))) return rc;
  if ((rc = c.stop.zero(h->stream))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  c.on = true;
  return MI_OSQP_OK;
}

// leave the continuous mode (a blocking call follows): wait for what is enqueued, forget the solves in flight
static int cont_leave(mi_osqp_batch *h) {
  mi_osqp_batch::Cont &c = h->cont;
  if (!c.on) return MI_OSQP_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t icnt = (size_t)h->ntiles * IS_COUNT * h->BT;
  HIPCHK(hipMemcpy(h->h_iscal, h->iscal.p, icnt * sizeof(int), hipMemcpyDeviceToHost));
  for (int q = 0; q < h->B; q++) {
    h->failed[q] = h->h_iscal[(size_t)(q / h->BT) * IS_COUNT * h->BT + IS_NEED_REFACTOR * h->BT + q % h->BT] < 0;
    if (c.clear_rho[q]) h->clear_rho_updates = true;      // (coarser than per QP, like the whole-batch update calls)
  }
  // the solutions of the finished QPs, for the whole-batch getters
  HIPCHK(hipMemcpy(h->x_out.p, c.xh, (size_t)h->B * (*h->anp).n * sizeof(double), hipMemcpyHostToDevice));
  if ((*h->anp).m) HIPCHK(hipMemcpy(h->y_out.p, c.yh, (size_t)h->B * (*h->anp).m * sizeof(double), hipMemcpyHostToDevice));
  if (any_cert_status(h))       // (a row is read under a status that wrote it: without such a status there is nothing to hand back)
    HIPCHK(hipMemcpy(h->cert_out.p, c.ch, (size_t)h->B * std::max(std::max((*h->anp).n, (*h->anp).m), 1) * sizeof(double), hipMemcpyHostToDevice));
  // every enqueued polish has run: those not reported yet have their result in the pinned image
  if (!h->st.polish) {
    bool any = !h->pol_status.empty();
    for (int q = 0; q < h->B; q++) {
      if (c.polishing[(size_t)q]) c.pol_status[(size_t)q] = c.h_pstat[q];
      any = any || c.pol_status[(size_t)q] != 0;
    }
    if (any) h->pol_status = c.pol_status;
  }
  c.on = false; c.n_running = 0;
  h->host_bounds_stale = h->host_rho_stale = true;
  return MI_OSQP_OK;
}

// a region of the staging ring: host pointer + the device address of the same offset
struct RingSpan { char *host; char *dev; };
static int ring_take(mi_osqp_batch *h, size_t bytes, RingSpan &out) {
  mi_osqp_batch::Cont &c = h->cont;
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes > c.ring_cap) { g_last_error = "per-QP call larger than the staging ring"; return MI_OSQP_ERR_ALLOC; }
  if (c.ring_head + bytes > c.ring_cap) { HIPCHK(hipStreamSynchronize(h->stream)); c.ring_head = 0; c.ring_wraps++; }      // everything handed out so far has been consumed
  out.host = c.ring_h + c.ring_head; out.dev = c.ring_d.p + c.ring_head;
  c.ring_head += bytes;
  return MI_OSQP_OK;
}
// Everything ONE call hands out must come from one lap of the ring.  A wrap between two spans of a call frees - at the wrap's
// synchronisation - nothing of the call's own earlier spans (they are filled and enqueued after it), and the head runs into
// them, unsynchronised, once it has advanced that far again: the staging of a QP's new rows could be overwritten while its
// transfer or its equilibration was still reading it (seen as a sporadic memory fault on the fourth run of 128 UR5e
// trajectories, whose updates take 140 KB of ring per QP).  So a call reserves its total first; the takes that follow cannot wrap.
static int ring_reserve(mi_osqp_batch *h, size_t bytes, int spans) {
  mi_osqp_batch::Cont &c = h->cont;
  bytes += (size_t)256 * (size_t)spans;
  if (bytes > c.ring_cap) { g_last_error = "per-QP call larger than the staging ring"; return MI_OSQP_ERR_ALLOC; }
  if (c.ring_head + bytes > c.ring_cap) { HIPCHK(hipStreamSynchronize(h->stream)); c.ring_head = 0; c.ring_wraps++; }
  return MI_OSQP_OK;
}
static int ring_upload(mi_osqp_batch *h, const RingSpan &sp, size_t bytes) {
  if (bytes) HIPCHK(hipMemcpyAsync(sp.dev, sp.host, bytes, hipMemcpyHostToDevice, h->stream));
  return MI_OSQP_OK;
}

static int cont_check_ids(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, bool must_be_idle) {
  if (n_ids < 0 || (n_ids > 0 && !ids)) return MI_OSQP_ERR_NULL;
  if (n_ids > h->B) return MI_OSQP_ERR_INVALID_DATA;
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) return MI_OSQP_ERR_INVALID_DATA;
    if (must_be_idle && h->cont.running[(size_t)ids[j]]) { g_last_error = "QP " + std::to_string(ids[j]) + " is still iterating"; return MI_OSQP_ERR_INVALID_DATA; }
  }
  return MI_OSQP_OK;
}

// the id list (as int) and, on request, the selection map of the tile kernels (slot -> position in the list + 1)
static int cont_stage_ids(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, int **d_ids, int **d_sel) {
  const int nslots = h->ntiles * h->BT;
  RingSpan sp;
  int rc = ring_take(h, ((size_t)n_ids + (d_sel ? (size_t)nslots : 0)) * sizeof(int), sp);
  if (rc) return rc;
  int *hi = (int *)sp.host;
  for (int64_t j = 0; j < n_ids; j++) hi[j] = (int)ids[j];
  if (d_sel) {
    int *hs = hi + n_ids;
    for (int sl = 0; sl < nslots; sl++) hs[sl] = 0;
    for (int64_t j = 0; j < n_ids; j++) hs[ids[j]] = (int)j + 1;        // (a QP listed twice: its last row wins)
    *d_sel = (int *)sp.dev + n_ids;
  }
  *d_ids = (int *)sp.dev;
  return ring_upload(h, sp, ((size_t)n_ids + (d_sel ? (size_t)nslots : 0)) * sizeof(int));
}

// the listed slots' share of the setup snapshot (mi_osqp_batch_reset restores it)
static int snapshot_some(mi_osqp_batch *h, const int *d_ids, int nq, hipStream_t st) {
  const Analysis &an = (*h->anp);
  HIPCHK(launch_copy_slot_streams(h->fwd_val0.p, h->fwd_val.p, d_ids, nq, (size_t)an.fwd.phys_steps() * 64, st));
  HIPCHK(launch_copy_slot_streams(h->bwd_val0.p, h->bwd_val.p, d_ids, nq, (size_t)an.bwd.phys_steps() * 64, st));
  if (an.dt.k) HIPCHK(launch_copy_slot_streams(h->dt_val0.p, h->dt_val.p, d_ids, nq, (size_t)an.dt.n_steps * 64, st));
  HIPCHK(launch_copy_slot_rows(h->dinv0.p, h->dinv.p, d_ids, nq, an.N, h->BT, st));
  HIPCHK(launch_copy_slot_rows(h->rho_vec0.p, h->rho_vec.p, d_ids, nq, an.m, h->BT, st));
  HIPCHK(launch_copy_slot_rows(h->rho_inv0.p, h->rho_inv.p, d_ids, nq, an.m, h->BT, st));
  HIPCHK(launch_copy_slot_rows(h->dscal0.p, h->dscal.p, d_ids, nq, DS_COUNT, h->BT, st));
  return MI_OSQP_OK;
}

// the refactorisation kernels for a device-resident work list of `count` entries (slots, -1 = none): one QP per workgroup,
// no group sharing (other handles' kernels may hold the CUs: nothing here may spin on a co-resident partner).
// pol != null: the polish factor of the listed slots instead, as in device_refactor_slots: into the polish buffers; the ADMM
// factor, the rho vectors and the flags stay as they are, a wrong inertia sets pol->stat[slot] = -1.
static int enqueue_refactor_list(mi_osqp_batch *h, const int *d_work, int count, const PolishArgs *pol = nullptr) {
  if (count <= 0) return MI_OSQP_OK;
  const Analysis &an = (*h->anp);
  hipStream_t st = h->stream;
  FactorArgs fa = make_factor_args(h, 0);
  fa.work = d_work; fa.mw_groups = 0;
  TailArgs da = make_tail_args(h, 1, d_work);
  if (pol) to_polish_factor(h, *pol, fa, da);
  HIPCHK(launch_factor(fa, 1, count, h->tune.factor_threads, st));
  if (an.dt.k) HIPCHK(launch_tail(da, count, h->dt_lds_asm, h->dt_lds, st));
  return MI_OSQP_OK;
}

// new A values + bounds of the listed QPs: equilibration on the device (fresh: from the raw P and q of setup; else unscale
// with the scaling in force first, as QPSolver::update does), check streams, refactorisation, snapshot.  All enqueued.
// (dA / dl / du non-null: the new data is on the device already, [B][nnzA] / [B][m] by QP number - the GOMP scene's kept rows)
// Pv non-null (fresh = false): new values of triu(P) as well, [n_ids][nnzP] in the analysis's order; the rawP rows of the
// listed QPs take them before the equilibration (a later reinit_some starts from them).  Av, l, u may then be null: A and the
// bounds stay (unscaled and rescaled), as in mi_osqp_batch_update_P.
static int cont_new_data(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *Av, const double *l, const double *u, bool fresh,
                         const double *dA = nullptr, const double *dl = nullptr, const double *du = nullptr, const double *Pv = nullptr) {
  const Analysis &an = (*h->anp);
  const int n = an.n, m = an.m, nnzP = an.Pp[n], nnzA = an.Ap[n], pa_len = nnzP + nnzA, nq = (int)n_ids;
  int rc;
  const bool hostA = !dA && Av;
  if (hostA) for (size_t k = 0; k < (size_t)nq * m; k++) if (l[k] > u[k]) return MI_OSQP_ERR_INVALID_DATA;
  int *d_ids = nullptr;
  const size_t cP = Pv ? (size_t)nq * nnzP : 0, cA = hostA ? (size_t)nq * nnzA : 0, cb = hostA ? (size_t)nq * m : 0, cpa = (size_t)nq * pa_len;
  const size_t cin = cP + cA + 2 * cb;          // one span: [P | A | l | u] rows of the call
  // (the whole call from one lap of the ring: ids, the rows in, the scaled values out)
  if ((rc = ring_reserve(h, (size_t)nq * sizeof(int) + cin * sizeof(double) + std::max<size_t>(cpa, 1) * sizeof(double), 3))) return rc;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, nullptr))) return rc;
  RingSpan in{nullptr, nullptr}, out;
  if (cin && (rc = ring_take(h, cin * sizeof(double), in))) return rc;
  if ((rc = ring_take(h, std::max<size_t>(cpa, 1) * sizeof(double), out))) return rc;
  double *hin = (double *)in.host, *din = (double *)in.dev;
  if (cin) {
    if (Pv) memcpy(hin, Pv, cP * sizeof(double));
    if (hostA) { memcpy(hin + cP, Av, cA * sizeof(double)); memcpy(hin + cP + cA, l, cb * sizeof(double)); memcpy(hin + cP + cA + cb, u, cb * sizeof(double)); }
    if ((rc = ring_upload(h, in, cin * sizeof(double)))) return rc;
  }
  hipStream_t us = h->stream;
  if (Pv) HIPCHK(launch_keep_rows(h->rawP.p, din, d_ids, nq, nnzP, us));
  if (hostA && h->cont.keepA) {
    HIPCHK(launch_keep_rows(h->cont.keepA, din + cP, d_ids, nq, nnzA, us));
    HIPCHK(launch_keep_rows(h->cont.keepl, din + cP + cA, d_ids, nq, m, us));
    HIPCHK(launch_keep_rows(h->cont.keepu, din + cP + cA + cb, d_ids, nq, m, us));
  }
  KernelArgs ka = make_args(h);
  if (fresh) HIPCHK(launch_fresh_slots(ka, d_ids, nq, h->BT, h->st.rho, us));
  RuizArgs r{};
  r.n = n; r.m = m; r.nnzP = nnzP; r.nnzA = nnzA; r.B = nq; r.BT = h->BT; r.iters = (int)h->st.scaling;
  r.ids = d_ids; r.fresh = fresh ? 1 : 0; r.rawP = h->rawP.p; r.rawq = h->rawq.p;
  r.Prow = h->rz_prow.p; r.Pcol = h->rz_pcol.p; r.Arow = h->rz_arow.p; r.Acol = h->rz_acol.p;
  if (Pv && !fresh) r.rawPnew = din;             // (row = position in the list, like every argument that comes with the call)
  if (dA) { r.rawA = dA; r.rawl = dl; r.rawu = du; r.raw_by_qp = 1; }
  else if (hostA) { r.rawA = din + cP; r.rawl = din + cP + cA; r.rawu = din + cP + cA + cb; }
  r.pa_val = h->pa_val.p; r.q = h->q.p; r.Dsc = h->Dsc.p; r.Dsc_inv = h->Dsc_inv.p; r.Esc = h->Esc.p; r.Esc_inv = h->Esc_inv.p;
  r.l = h->l.p; r.u = h->u.p; r.dscal = h->dscal.p;
  r.dn = h->cont.rz_scratch.p; r.en = h->cont.rz_scratch.p + (size_t)h->B * n;        // (not the check kernels' scratch: they may be running)
  r.pa_out = (double *)out.dev;
  HIPCHK(launch_ruiz(r, us));
  HIPCHK(launch_scatter(r.pa_out, h->chk_val.p, h->chk.src.p, d_ids, nq, pa_len, h->chk.view(an.chk), h->BT, us));
  if ((rc = enqueue_refactor_list(h, d_ids, nq))) return rc;
  if ((rc = snapshot_some(h, d_ids, nq, us))) return rc;
  for (int64_t j = 0; j < n_ids; j++) { h->cont.clear_rho[(size_t)ids[j]] = 1; h->failed[(size_t)ids[j]] = 0; h->cont.polishable[(size_t)ids[j]] = 0; }
  if (fresh) for (int64_t j = 0; j < n_ids; j++) h->cont.cert_status[(size_t)ids[j]] = 0;      // (a new QP in the slot: it has not finished a solve)
  h->host_scaling_stale = true; h->host_bounds_stale = true; h->host_rho_stale = true;
  return MI_OSQP_OK;
}
// the listed ids once each (the per-QP P updates: two rows for one QP have no defined winner in rawP)
static int cont_check_unique(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids) {
  std::vector<char> seen((size_t)h->B, 0);
  for (int64_t j = 0; j < n_ids; j++) {
    if (seen[(size_t)ids[j]]) { g_last_error = "QP " + std::to_string(ids[j]) + " is listed twice"; return MI_OSQP_ERR_INVALID_DATA; }
    seen[(size_t)ids[j]] = 1;
  }
  return MI_OSQP_OK;
}

extern "C" {

int mi_osqp_batch_reinit_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *Av, const double *l, const double *u) {
  CallTimer timer_("batch_reinit_some");
  if (!h || (n_ids > 0 && (!Av || !l || !u))) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  return cont_new_data(h, n_ids, ids, Av, l, u, true);
}

int mi_osqp_batch_update_A_bounds_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *Av, const double *l, const double *u) {
  CallTimer timer_("batch_update_A_bounds_some");
  if (!h || (n_ids > 0 && (!Av || !l || !u))) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  return cont_new_data(h, n_ids, ids, Av, l, u, false);
}

// osqp_update_P (and QPSolver::update) for the listed (idle) QPs: ring upload, the rawP rows, equilibration, refactorisation
// and snapshot of those QPs; nothing waits
int mi_osqp_batch_update_P_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *Pv) {
  CallTimer timer_("batch_update_P_some");
  if (!h || (n_ids > 0 && !Pv)) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true)) || (rc = cont_check_unique(h, n_ids, ids))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  return cont_new_data(h, n_ids, ids, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr, Pv);
}

int mi_osqp_batch_update_P_A_bounds_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *Pv, const double *Av,
                                         const double *l, const double *u) {
  CallTimer timer_("batch_update_P_A_bounds_some");
  if (!h || (n_ids > 0 && (!Pv || !Av || !l || !u))) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true)) || (rc = cont_check_unique(h, n_ids, ids))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  return cont_new_data(h, n_ids, ids, Av, l, u, false, nullptr, nullptr, nullptr, Pv);
}

int mi_osqp_batch_warm_start_x_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *x) {
  CallTimer timer_("batch_warm_start_x_some");
  if (!h || (n_ids > 0 && !x)) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  h->st.warm_start = 1;
  const size_t cnt = (size_t)n_ids * (*h->anp).n;
  int *d_ids = nullptr, *d_sel = nullptr;
  RingSpan sp;
  if ((rc = ring_reserve(h, ((size_t)n_ids + (size_t)h->ntiles * h->BT) * sizeof(int) + cnt * sizeof(double), 2))) return rc;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, &d_sel)) || (rc = ring_take(h, cnt * sizeof(double), sp))) return rc;
  memcpy(sp.host, x, cnt * sizeof(double));
  if ((rc = ring_upload(h, sp, cnt * sizeof(double)))) return rc;
  KernelArgs a = make_args(h);
  a.sel = d_sel;
  HIPCHK(launch_warm_start(a, h->BT, h->ntiles, h->threads, h->lds, h->stream, (const double *)sp.dev));
  for (int64_t j = 0; j < n_ids; j++) h->cont.polishable[(size_t)ids[j]] = 0;
  return MI_OSQP_OK;
}

// osqp_update_lin_cost for the listed (idle) QPs: ring upload, lin_cost_kernel, nothing waits
int mi_osqp_batch_update_q_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *q) {
  CallTimer timer_("batch_update_q_some");
  if (!h || (n_ids > 0 && !q)) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  const int n = (*h->anp).n;
  const size_t cnt = (size_t)n_ids * n;
  int *d_ids = nullptr;
  RingSpan sp;
  if ((rc = ring_reserve(h, (size_t)n_ids * sizeof(int) + cnt * sizeof(double), 2))) return rc;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, nullptr)) || (rc = ring_take(h, cnt * sizeof(double), sp))) return rc;
  memcpy(sp.host, q, cnt * sizeof(double));
  if ((rc = ring_upload(h, sp, cnt * sizeof(double)))) return rc;
  HIPCHK(launch_lin_cost((const double *)sp.dev, d_ids, h->q.p, h->rawq.p, h->Dsc.p, h->dscal.p, (int)n_ids, n, h->BT,
                         h->st.scaling ? 1 : 0, h->stream));
  for (int64_t j = 0; j < n_ids; j++) { h->cont.clear_rho[(size_t)ids[j]] = 1; h->cont.polishable[(size_t)ids[j]] = 0; }
  h->host_scaling_stale = true;
  return MI_OSQP_OK;
}

// osqp_warm_start_y for the listed (idle) QPs
int mi_osqp_batch_warm_start_y_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *y) {
  CallTimer timer_("batch_warm_start_y_some");
  if (!h || (n_ids > 0 && !y)) return MI_OSQP_ERR_NULL;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  h->st.warm_start = 1;
  const size_t cnt = (size_t)n_ids * (*h->anp).m;
  int *d_ids = nullptr, *d_sel = nullptr;
  RingSpan sp;
  if ((rc = ring_reserve(h, ((size_t)n_ids + (size_t)h->ntiles * h->BT) * sizeof(int) + cnt * sizeof(double), 2))) return rc;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, &d_sel)) || (rc = ring_take(h, std::max<size_t>(cnt, 1) * sizeof(double), sp))) return rc;
  memcpy(sp.host, y, cnt * sizeof(double));
  if ((rc = ring_upload(h, sp, cnt * sizeof(double)))) return rc;
  KernelArgs a = make_args(h);
  a.sel = d_sel;
  HIPCHK(launch_warm_start_y(a, h->ntiles * h->BT, h->BT, h->stream, (const double *)sp.dev));
  for (int64_t j = 0; j < n_ids; j++) h->cont.polishable[(size_t)ids[j]] = 0;
  return MI_OSQP_OK;
}

int mi_osqp_batch_solve_begin_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids) {
  CallTimer timer_("batch_solve_begin_some");
  if (!h) return MI_OSQP_ERR_NULL;
  if (h->st.polish) { g_last_error = "the continuous mode does not polish: set up the handle with polish = 0"; return MI_OSQP_ERR_INVALID_SETTINGS; }
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  mi_osqp_batch::Cont &c = h->cont;
  RingSpan sp;
  if ((rc = ring_take(h, 2 * (size_t)n_ids * sizeof(int), sp))) return rc;
  int *hi = (int *)sp.host;
  for (int64_t j = 0; j < n_ids; j++) {
    const size_t q = (size_t)ids[j];
    hi[j] = (int)q; hi[n_ids + j] = c.clear_rho[q] ? 1 : 0;
    c.clear_rho[q] = 0;
  }
  if ((rc = ring_upload(h, sp, 2 * (size_t)n_ids * sizeof(int)))) return rc;
  KernelArgs a = make_args(h);
  a.x_out = c.xh; a.y_out = c.yh; a.cert_out = c.ch;
  // (a QP whose last refactorisation lost the inertia carries flag -1 on the device: start_slots_kernel ends it as kNonConvex)
  HIPCHK(launch_start_slots(a, (const int *)sp.dev, (const int *)sp.dev + n_ids, (int)n_ids, h->BT, h->st.warm_start ? 0 : 1, h->stream));
  for (int64_t j = 0; j < n_ids; j++) {
    const size_t q = (size_t)ids[j];
    if (!c.running[q]) { c.running[q] = 1; c.n_running++; }
    c.epoch[q]++;
    c.polishable[q] = 0; c.pol_status[q] = 0;
    c.cert_status[q] = 0;                 // (the solve in flight writes the QP's certificate row when it finishes)
  }
  return MI_OSQP_OK;
}

// Polish the listed QPs - finished, reported kOptimal by poll() and untouched since - without waiting for the device
// (mi_osqp.h): active set of the listed slots, their polish factors (one QP per workgroup, the list path of the
// refactorisations), polish_kernel over the tiles (a tile without a marked QP leaves at once; the tile partner of a polished
// QP may be in the middle of its solve: the kernel stores to the marked QPs only, and the tile scratch it uses - out1, out2,
// pol_sol - is ordered against the advance launches by the stream), publication.  All or nothing as far as refusals go: a
// refused call has enqueued and changed nothing (a HIP error in the middle of the chain is not a refusal: like every
// MI_OSQP_ERR_DEVICE it leaves the handle's device state undefined, here with marks that may still be up).  The QPs count as running until the poll of the next advance reports them a second time: the epoch
// the publication kernel moves is what tells that report from the one of the solve (an advance enqueued BEFORE this call
// publishes the old epoch and reports nothing).  The marks (pol_stat = 1) are up only within one call's chain, so a second
// call before the report neither polishes the first call's QPs again nor loses their results (the pinned image keeps them).
int mi_osqp_batch_polish_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids) {
  CallTimer timer_("batch_polish_some");
  if (!h || (n_ids > 0 && !ids)) return MI_OSQP_ERR_NULL;
  mi_osqp_batch::Cont &c = h->cont;
  if (!c.on) { g_last_error = "polish_some: the handle is not in the continuous mode"; return MI_OSQP_ERR_INVALID_DATA; }
  if (n_ids < 0 || n_ids > h->B) { g_last_error = "polish_some: more ids than QPs"; return MI_OSQP_ERR_INVALID_DATA; }
  if (!n_ids) return MI_OSQP_OK;
  {
    std::vector<char> seen((size_t)h->B, 0);
    for (int64_t j = 0; j < n_ids; j++) {
      const int64_t q = ids[j];
      const char *why = nullptr;
      if (q < 0 || q >= h->B) why = " is out of range";
      else if (seen[(size_t)q]) why = " is listed twice";
      else if (c.running[(size_t)q]) why = " is still running";
      else if (!c.polishable[(size_t)q]) why = " is not polishable (not reported kOptimal, changed since, or polished already)";
      if (why) { g_last_error = "polish_some: QP " + std::to_string(q) + why; return MI_OSQP_ERR_INVALID_DATA; }
      seen[(size_t)q] = 1;
    }
  }
  DevGuard guard(h->device);
  int rc;
  const int BT = h->BT, nq = (int)n_ids;
  if ((rc = ensure_polish_buffers(h))) return rc;           // (the one-time allocation: the only thing here that may wait)
  if (!c.h_pstat) {
    HIPCHK(hostpool::alloc((void **)&c.h_pstat, (size_t)h->ntiles * BT * sizeof(int), &c.h_pstat_cap));
    for (int s = 0; s < h->ntiles * BT; s++) c.h_pstat[s] = 0;
  }
  int *d_ids = nullptr;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, nullptr))) return rc;
  KernelArgs a = make_args(h);
  a.x_out = c.xh; a.y_out = c.yh; a.cert_out = c.ch;
  PolishArgs pa{h->pol_stat.p, h->pol_act.p, h->pol_sol.p, (int)h->st.polish_refine_iter, kPolishInner, h->st.delta};
  HIPCHK(launch_polish_active_list(a, pa, d_ids, nq, BT, h->stream));
  if ((rc = enqueue_refactor_list(h, d_ids, nq, &pa))) return rc;
  HIPCHK(launch_polish(polish_stream_args(h, a), pa, BT, h->ntiles, h->threads, h->lds, h->n_cus, h->stream));
  HIPCHK(launch_polish_publish(a, pa, d_ids, nq, c.h_pstat, BT, h->stream));
  for (int64_t j = 0; j < n_ids; j++) {
    const size_t q = (size_t)ids[j];
    c.polishable[q] = 0; c.polishing[q] = 1;
    c.running[q] = 1; c.n_running++;
    c.epoch[q]++;
  }
  return MI_OSQP_OK;
}

int mi_osqp_batch_advance(mi_osqp_batch *h, int64_t n_segments) {
  CallTimer timer_("batch_advance");
  if (!h) return MI_OSQP_ERR_NULL;
  if (n_segments <= 0) return MI_OSQP_ERR_INVALID_DATA;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h))) return rc;
  mi_osqp_batch::Cont &c = h->cont;
  if (c.adv_seq - c.polled_seq >= 2) { g_last_error = "advance: two advances are waiting for poll()"; return MI_OSQP_ERR_INVALID_DATA; }
  const int BT = h->BT, nslots = h->ntiles * BT;
  KernelArgs a = make_args(h);
  a.x_out = c.xh; a.y_out = c.yh; a.cert_out = c.ch;
  // ONE launch: every tile runs up to n_segments segments (L iterations + check each) and publishes its flags and the
  // solutions of finished QPs in pinned host memory; with several segments the launch ends early for everybody once a QP
  // has finished (the caller wants to react to it), and for a tile whose QP asks for a refactorisation
  a.info_at_end = 1;
  c.launch_seq++;
  const int par = (int)(c.adv_seq & 1);
  HIPCHK(launch_advance(a, BT, h->ntiles, h->threads, h->lds_iter, h->stream, (int)std::min<int64_t>(n_segments, 1 << 20), c.L, c.h_is[par], c.h_ds[par],
                        n_segments > 1 ? c.stop.p : nullptr, c.launch_seq, c.counter.p, c.h_done));
  HIPCHK(hipEventRecord(c.ev[par], h->stream));
  if (h->st.adaptive_rho) {
    // row E13 without the host, next to the following launches: the QPs this launch paused (their rho changed) are listed on
    // the device, refactored and marked to resume - or ended as kNonConvex when the new factor lost its inertia
    HIPCHK(launch_worklist(h->iscal.p, c.work.p, nslots, BT, h->stream));
    if ((rc = enqueue_refactor_list(h, c.work.p, nslots))) return rc;
    HIPCHK(launch_resume_flagged(a, nslots, BT, h->stream));
  }
  c.adv_seq++;
  c.seq_of[par] = c.adv_seq;
  h->host_rho_stale = true;
  return MI_OSQP_OK;
}

int mi_osqp_batch_poll(mi_osqp_batch *h, int64_t wait, int64_t *n_finished, int64_t *ids_out, int64_t capacity) {
  CallTimer timer_("batch_poll");
  if (!h || !n_finished) return MI_OSQP_ERR_NULL;
  *n_finished = 0;
  mi_osqp_batch::Cont &c = h->cont;
  if (!c.on || c.polled_seq >= c.adv_seq) return MI_OSQP_OK;      // nothing enqueued
  DevGuard guard(h->device);
  const int64_t seq = c.polled_seq + 1;
  const int par = (int)((seq - 1) & 1);
  // the launch is over when its last tile has written the sequence number into pinned memory (no runtime call in the way:
  // waking up from hipEventSynchronize costs up to milliseconds when several host threads wait on several streams)
  auto over = [&]() { return __atomic_load_n(c.h_done, __ATOMIC_ACQUIRE) >= (unsigned)seq; };
  if (!over()) {
    if (!wait) { *n_finished = -1; return MI_OSQP_OK; }
    const double t0 = now_s();
    for (int spin = 0; !over(); spin++) {
      if (spin < 2000) { __builtin_ia32_pause(); continue; }
      struct timespec ts{0, 20000};                      // 20 us
      nanosleep(&ts, nullptr);
      if ((spin & 1023) == 0 && now_s() - t0 > 5.0) { HIPCHK(hipEventSynchronize(c.ev[par])); if (!over()) { g_last_error = "advance launch ended without reporting"; return MI_OSQP_ERR_DEVICE; } }
    }
  }
  const int BT = h->BT;
  int64_t nf = 0;
  auto finished = [&](int q) {
    if (!c.running[q]) return false;
    const int *ti = c.h_is[par] + (size_t)(q / BT) * IS_COUNT * BT;
    const int b = q % BT;
    return ti[IS_DONE * BT + b] != 0 && ti[IS_PENDING * BT + b] == 0 && ti[IS_EPOCH * BT + b] == c.epoch[(size_t)q];
  };
  // (the caller's buffer must take every finished QP of this advance: with less room nothing is consumed)
  int64_t would = 0, n_pol = 0, n_acc = 0;
  for (int q = 0; q < h->B; q++) would += finished(q) ? 1 : 0;
  if (would > capacity || (would > 0 && !ids_out)) { *n_finished = would; g_last_error = "poll: ids_out too small"; return MI_OSQP_ERR_INVALID_DATA; }
  for (int q = 0; q < h->B; q++) {
    if (!finished(q)) continue;
    const int *ti = c.h_is[par] + (size_t)(q / BT) * IS_COUNT * BT;
    const int b = q % BT;
    const double *td = c.h_ds[par] + (size_t)(q / BT) * DS_COUNT * BT;
    mi_osqp_info &I = c.info[(size_t)q];
    I.iter = ti[IS_ITER * BT + b]; I.status_val = ti[IS_STATUS * BT + b]; I.exit_code = exit_code_of((int)I.status_val);
    I.obj_val = td[DS_OBJ * BT + b]; I.pri_res = td[DS_PRI_RES * BT + b]; I.dua_res = td[DS_DUA_RES * BT + b];
    I.rho_updates = ti[IS_RHO_UPDATES * BT + b]; I.rho_estimate = td[DS_RHO_EST * BT + b]; I.rho = td[DS_RHO * BT + b];
    if (ti[IS_NEED_REFACTOR * BT + b] < 0) h->failed[(size_t)q] = 1;
    c.cert_status[(size_t)q] = (int)I.status_val;
    if (c.polishing[(size_t)q]) {      // the second report of a polished QP: (the image is valid: the epoch moved after it was written)
      c.polishing[(size_t)q] = 0;
      c.pol_status[(size_t)q] = c.h_pstat[q];
      n_pol++; n_acc += c.h_pstat[q] == 1;
    } else {
      c.pol_status[(size_t)q] = 0;
      c.polishable[(size_t)q] = I.status_val == 1;
    }
    I.status_polish = c.pol_status[(size_t)q];
    c.running[q] = 0; c.n_running--;
    ids_out[nf++] = q;
  }
  if (n_pol) { h->pol_count = n_pol; h->pol_accepted = n_acc; h->pol_seconds = 0.0; }
  c.polled_seq = seq;
  *n_finished = nf;
  return MI_OSQP_OK;
}

int mi_osqp_batch_get_primal_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *x_out) {
  if (!h || (n_ids > 0 && (!ids || !x_out))) return MI_OSQP_ERR_NULL;
  if (!h->cont.on) return MI_OSQP_ERR_INVALID_DATA;
  const size_t n = (size_t)(*h->anp).n;
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) return MI_OSQP_ERR_INVALID_DATA;
    memcpy(x_out + (size_t)j * n, h->cont.xh + (size_t)ids[j] * n, n * sizeof(double));
  }
  return MI_OSQP_OK;
}
int mi_osqp_batch_get_dual_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *y_out) {
  if (!h || (n_ids > 0 && (!ids || !y_out))) return MI_OSQP_ERR_NULL;
  if (!h->cont.on) return MI_OSQP_ERR_INVALID_DATA;
  const size_t m = (size_t)(*h->anp).m;
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) return MI_OSQP_ERR_INVALID_DATA;
    memcpy(y_out + (size_t)j * m, h->cont.yh + (size_t)ids[j] * m, m * sizeof(double));
  }
  return MI_OSQP_OK;
}
int mi_osqp_batch_get_info_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, mi_osqp_info *info) {
  if (!h || (n_ids > 0 && (!ids || !info))) return MI_OSQP_ERR_NULL;
  if (!h->cont.on) return MI_OSQP_ERR_INVALID_DATA;
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) return MI_OSQP_ERR_INVALID_DATA;
    info[j] = h->cont.info[(size_t)ids[j]];
  }
  return MI_OSQP_OK;
}
// (the status is the one poll() reported for the QP's last finished solve, until its next solve begins or the slot is
//  reinitialised: Cont::cert_status; no device is touched)
static int get_cert_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *out, bool primal) {
  if (!h || (n_ids > 0 && (!ids || !out))) return MI_OSQP_ERR_NULL;
  if (!h->cont.on) return MI_OSQP_ERR_INVALID_DATA;
  const size_t n = (size_t)(*h->anp).n, m = (size_t)(*h->anp).m, len = primal ? m : n, stride = std::max(std::max(n, m), (size_t)1);
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) return MI_OSQP_ERR_INVALID_DATA;
    cert_row(out + (size_t)j * len, h->cont.ch + (size_t)ids[j] * stride, len, cert_status(h->cont.cert_status[(size_t)ids[j]], primal));
  }
  return MI_OSQP_OK;
}
int mi_osqp_batch_get_prim_inf_cert_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *dy_out) {
  return get_cert_some(h, n_ids, ids, dy_out, true);
}
int mi_osqp_batch_get_dual_inf_cert_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, double *dx_out) {
  return get_cert_some(h, n_ids, ids, dx_out, false);
}
int64_t mi_osqp_batch_running(mi_osqp_batch *h) { return h && h->cont.on ? h->cont.n_running : 0; }
int64_t mi_osqp_batch_ring_wraps(mi_osqp_batch *h) { return h ? h->cont.ring_wraps : 0; }

}  // extern "C"

// ------------------------------------------------------------------ settings updates
// OSQP 0.6.x osqp_update_* (README "Settings updates").  Every field but rho is read by the host loop / passed to the kernels
// with each launch (make_args), so storing it is the whole update; a new rho is osqp_update_rho: DS_RHO of the QPs
// (set_rho_slots_kernel), the refactorisation that derives the rho vectors from it, the snapshot mi_osqp_batch_reset returns
// to.  Iterates and the count of rho updates stay (upstream restarts the count in data updates only).

static mi_osqp_settings from_settings(const Settings &t) {
  mi_osqp_settings s;
  s.rho = t.rho; s.sigma = t.sigma; s.scaling = t.scaling; s.adaptive_rho = t.adaptive_rho;
  s.adaptive_rho_interval = t.adaptive_rho_interval; s.adaptive_rho_tolerance = t.adaptive_rho_tolerance;
  s.max_iter = t.max_iter; s.eps_abs = t.eps_abs; s.eps_rel = t.eps_rel; s.eps_prim_inf = t.eps_prim_inf;
  s.eps_dual_inf = t.eps_dual_inf; s.alpha = t.alpha; s.scaled_termination = t.scaled_termination;
  s.check_termination = t.check_termination; s.warm_start = t.warm_start; s.verbose = t.verbose;
  s.polish = t.polish; s.polish_refine_iter = t.polish_refine_iter; s.delta = t.delta;
  return s;
}
static double clamp_rho(double r) { return std::min(std::max(r, kRhoMin), kRhoMax); }

// May `w` replace `cur`?  The fields without an osqp_update_* must be those in force (adaptive_rho_interval = 0 stands for the
// interval setup resolved "auto" to), the rest must be valid.  The reason of a refusal goes to g_last_error.
static int settings_update_decide(const mi_osqp_settings &cur, const mi_osqp_settings &w) {
  const char *fixed = nullptr;
  if (!(w.sigma == cur.sigma)) fixed = "sigma";
  else if (w.scaling != cur.scaling) fixed = "scaling";
  else if (w.adaptive_rho != cur.adaptive_rho) fixed = "adaptive_rho";
  else if (w.adaptive_rho_interval != cur.adaptive_rho_interval && w.adaptive_rho_interval != 0) fixed = "adaptive_rho_interval";
  else if (!(w.adaptive_rho_tolerance == cur.adaptive_rho_tolerance)) fixed = "adaptive_rho_tolerance";
  if (fixed) { g_last_error = std::string("settings update: ") + fixed + " is fixed at setup"; return MI_OSQP_ERR_INVALID_SETTINGS; }
  Settings t = to_settings(&w);
  t.adaptive_rho_interval = cur.adaptive_rho_interval;
  if (validate_settings(t)) { g_last_error = "settings update: a value is out of range (nothing changed)"; return MI_OSQP_ERR_INVALID_SETTINGS; }
  return MI_OSQP_OK;
}

static int check_rho_values(int64_t count, const double *rho) {
  for (int64_t j = 0; j < count; j++)
    if (!(rho[j] > 0.0)) { g_last_error = "rho update: entry " + std::to_string(j) + " is not > 0 (nothing changed)"; return MI_OSQP_ERR_INVALID_SETTINGS; }
  return MI_OSQP_OK;
}

// blocking form: rho of every QP (rho_each[B], or rho_all), one refactorisation of the whole batch, the snapshot
static int set_rho_blocking(mi_osqp_batch *h, const double *rho_each, double rho_all) {
  const int B = h->B;
  int rc;
  const double *d_rho = nullptr;
  if (rho_each) {
    if ((rc = ensure_stage(h, (size_t)B, 0)) || (rc = ensure_pin(h, (size_t)B))) return rc;
    for (int q = 0; q < B; q++) h->pin[q] = clamp_rho(rho_each[q]);
    HIPCHK(hipMemcpyAsync(h->stage.p, h->pin, (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    d_rho = h->stage.p;
  }
  HIPCHK(launch_set_rho_slots(make_args(h), nullptr, d_rho, rho_all, B, h->BT, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->host_rho_stale = true;
  std::vector<int> all(B);
  for (int i = 0; i < B; i++) all[i] = i;
  if ((rc = refactor_qps(h, std::move(all)))) return rc;          // (the one-launch list path: factor_kernel derives the rho vectors)
  return snapshot(h);
}

// continuous form, for idle QPs: enqueued in stream order behind everything enqueued so far, nothing waits.  The ids have
// been checked (cont_check_ids, no repeats), the values too.
static int set_rho_continuous(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *rho) {
  const int nq = (int)n_ids;
  int rc;
  int *d_ids = nullptr;
  RingSpan sp;
  if ((rc = ring_reserve(h, (size_t)nq * (sizeof(int) + sizeof(double)), 2))) return rc;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, nullptr)) || (rc = ring_take(h, (size_t)nq * sizeof(double), sp))) return rc;
  for (int j = 0; j < nq; j++) ((double *)sp.host)[j] = clamp_rho(rho[j]);
  if ((rc = ring_upload(h, sp, (size_t)nq * sizeof(double)))) return rc;
  HIPCHK(launch_set_rho_slots(make_args(h), d_ids, (const double *)sp.dev, 0.0, nq, h->BT, h->stream));
  if ((rc = enqueue_refactor_list(h, d_ids, nq))) return rc;
  if ((rc = snapshot_some(h, d_ids, nq, h->stream))) return rc;
  for (int64_t j = 0; j < n_ids; j++) { h->failed[(size_t)ids[j]] = 0; h->cont.polishable[(size_t)ids[j]] = 0; }
  h->host_rho_stale = true;
  return MI_OSQP_OK;
}

extern "C" {

int mi_osqp_settings_update_check(const mi_osqp_settings *in_force, const mi_osqp_settings *wanted) {
  if (!in_force || !wanted) return MI_OSQP_ERR_NULL;
  return settings_update_decide(*in_force, *wanted);
}

int mi_osqp_batch_get_settings(mi_osqp_batch *h, mi_osqp_settings *out) {
  if (!h || !out) return MI_OSQP_ERR_NULL;
  *out = from_settings(h->st);
  return MI_OSQP_OK;
}

int mi_osqp_batch_update_settings(mi_osqp_batch *h, const mi_osqp_settings *s) {
  CallTimer timer_("batch_update_settings");
  if (!h || !s) return MI_OSQP_ERR_NULL;
  const mi_osqp_settings cur = from_settings(h->st);
  int rc;
  if ((rc = settings_update_decide(cur, *s))) return rc;
  if (s->adaptive_rho_interval == 0 && cur.adaptive_rho_interval != 0 && !h->rho_interval_auto) {
    g_last_error = "settings update: adaptive_rho_interval is fixed at setup (0 is accepted where setup derived it from 0)";
    return MI_OSQP_ERR_INVALID_SETTINGS;
  }
  mi_osqp_batch::Cont &c = h->cont;
  if (c.on && c.n_running > 0) {
    g_last_error = "settings update: " + std::to_string(c.n_running) + " QPs are running (poll them first)";
    return MI_OSQP_ERR_INVALID_DATA;
  }
  const bool new_rho = s->rho != h->st.rho;
  const double rho = clamp_rho(s->rho);
  Settings t = to_settings(s);
  t.sigma = h->st.sigma; t.scaling = h->st.scaling; t.adaptive_rho = h->st.adaptive_rho;
  t.adaptive_rho_interval = h->st.adaptive_rho_interval; t.adaptive_rho_tolerance = h->st.adaptive_rho_tolerance;
  t.rho = new_rho ? rho : h->st.rho;
  h->st = t;
  if (c.on) c.L = segment_length(h->st);
  if (!new_rho) return MI_OSQP_OK;
  DevGuard guard(h->device);
  if (!c.on) return set_rho_blocking(h, nullptr, rho);
  std::vector<int64_t> ids((size_t)h->B);
  for (int q = 0; q < h->B; q++) ids[(size_t)q] = q;
  const std::vector<double> each((size_t)h->B, rho);
  return set_rho_continuous(h, h->B, ids.data(), each.data());
}

int mi_osqp_batch_update_rho_each(mi_osqp_batch *h, const double *rho) {
  CallTimer timer_("batch_update_rho_each");
  if (!h || !rho) return MI_OSQP_ERR_NULL;
  int rc;
  if ((rc = check_rho_values(h->B, rho))) return rc;
  DevGuard guard(h->device);
  if ((rc = cont_leave(h))) return rc;
  return set_rho_blocking(h, rho, 0.0);
}

int mi_osqp_batch_update_rho_some(mi_osqp_batch *h, int64_t n_ids, const int64_t *ids, const double *rho) {
  CallTimer timer_("batch_update_rho_some");
  if (!h || (n_ids > 0 && !rho)) return MI_OSQP_ERR_NULL;
  int rc;
  if ((rc = check_rho_values(n_ids, rho))) return rc;
  DevGuard guard(h->device);
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  if (!n_ids) return MI_OSQP_OK;
  {
    std::vector<char> seen((size_t)h->B, 0);
    for (int64_t j = 0; j < n_ids; j++) {
      if (seen[(size_t)ids[j]]) { g_last_error = "update_rho_some: QP " + std::to_string(ids[j]) + " is listed twice"; return MI_OSQP_ERR_INVALID_DATA; }
      seen[(size_t)ids[j]] = 1;
    }
  }
  return set_rho_continuous(h, n_ids, ids, rho);
}

}  // extern "C"

// ------------------------------------------------------------------ gomp scene
// SURVEY 8(f) rank 2 on the device: the re-linearised 3-D / obstacle rows of the GOMP constraint matrix
// ([REF] src/constraints/constraint-builder.h:90-136) and the feasibility check that decides the SQP loop
// ([REF] src/gomp-solver.h:141-199), for balls whose kinematics are built-in models.  The scene keeps the raw constraint
// data of every QP of a batch handle on the device; re-linearising a QP rewrites its 3-D rows there (gomp_relinearise_kernel)
// and runs QPSolver::update from them - no A values cross PCIe in an SQP step, only the trajectory (n doubles) and one flag.
// Besides the built-in models a scene may hold one DH chain (mi_gomp_chain) with balls fixed in its link frames.
struct mi_gomp_scene {
  mi_osqp_batch *h = nullptr;
  int dims = 0, W = 0, n_balls = 0, n_lines = 0, n_caps = 0, n_cuboids = 0, n_pairs = 0, pair_row0 = 0, n_tilts = 0, tilt_row0 = 0, row0 = 0, n_rows3d = 0, n_grids = 0, n_goals = 0, goal_row0 = 0;
  double con_lo[3] = {-1e30, -1e30, -1e30}, con_hi[3] = {1e30, 1e30, 1e30};
  DevBuf<GompBallDev> balls;
  DevBuf<GompLineDev> lines;
  DevBuf<GompCapsuleDev> caps;
  DevBuf<GompCuboidDev> cuboids;
  DevBuf<GompPairDev> pairs;                  // their rows: pair_row0 + k W + w, behind every ball's block
  DevBuf<GompTiltDev> tilts;                  // their rows: tilt_row0 + k W + w, behind the pair rows
  DevBuf<GompGridDev> grids;                  // distance grids: their rows follow the cuboids' in every (ball, waypoint) block
  DevBuf<double> grid_vals;                   // the nodes of all grids, one after the other
  std::vector<size_t> grid_off, grid_len;     // where grid k's nodes start in grid_vals and how many they are
  DevBuf<GompGoalDev> goals;                  // grasp goals: their rows goal_row0 + 4 k + r, behind the tilt rows
  DevBuf<GompGoalValDev> goal_vals;           // [B][n_goals]: what each QP asks of the goals (mi_gomp_scene_set_goal_values)
  std::vector<int> goal_frame;                // the goals' frames, for the checks of the values
  std::vector<char> goal_set;                 // [B]: this QP's values have been set
  GompChainDev chain{};                       // the DH chain of the MI_GM_DH_CHAIN balls (n_joints 0: the scene has none)
  DevBuf<int> aidx;
  DevBuf<double> A, l, u;                     // QP-major raw rows as ConstraintBuilder::build() lays them out
  int *h_ok = nullptr; size_t h_ok_cap = 0;   // the kernel's verdicts (pinned host memory)
  hipEvent_t ev = nullptr;
  ~mi_gomp_scene() { hostpool::give(h_ok, h_ok_cap); if (ev) (void)hipEventDestroy(ev); }
};

static int gomp_launch(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *x, int write_rows /* 0 never, 1 always, 2 unless accepted */, int32_t *ok_out) {
  mi_osqp_batch *h = sc->h;
  const Analysis &an = (*h->anp);
  const int n = an.n, m = an.m, nq = (int)n_ids;
  int rc;
  // trajectories and ids through the handle's staging ring (pinned, asynchronous), the verdicts straight into pinned host memory
  int *d_ids = nullptr;
  RingSpan sp;
  if ((rc = ring_reserve(h, (size_t)nq * sizeof(int) + (size_t)nq * n * sizeof(double), 2))) return rc;
  if ((rc = cont_stage_ids(h, n_ids, ids, &d_ids, nullptr)) || (rc = ring_take(h, (size_t)nq * n * sizeof(double), sp))) return rc;
  memcpy(sp.host, x, (size_t)nq * n * sizeof(double));
  if ((rc = ring_upload(h, sp, (size_t)nq * n * sizeof(double)))) return rc;
  hipStream_t st = h->stream;
  GompArgs g{};
  g.dims = sc->dims; g.W = sc->W; g.n_balls = sc->n_balls; g.n_lines = sc->n_lines; g.n_caps = sc->n_caps; g.n_cuboids = sc->n_cuboids; g.n_pairs = sc->n_pairs; g.pair_row0 = sc->pair_row0; g.n_tilts = sc->n_tilts; g.tilt_row0 = sc->tilt_row0; g.n_grids = sc->n_grids; g.n_goals = sc->n_goals; g.goal_row0 = sc->goal_row0; g.n = n; g.m = m; g.nnzA = an.Ap[n]; g.n_ids = nq;
  g.row0 = sc->row0; g.write_rows = write_rows;
  g.ids = d_ids; g.balls = sc->balls.p; g.lines = sc->lines.p; g.caps = sc->caps.p; g.cuboids = sc->cuboids.p; g.pairs = sc->pairs.p; g.tilts = sc->tilts.p; g.grids = sc->grids.p; g.goals = sc->goals.p; g.goal_vals = sc->goal_vals.p; g.aidx = sc->aidx.p; g.traj = (const double *)sp.dev;
  for (int k = 0; k < 3; k++) { g.con_lo[k] = sc->con_lo[k]; g.con_hi[k] = sc->con_hi[k]; }
  g.A = sc->A.p; g.l = sc->l.p; g.u = sc->u.p; g.ok = sc->h_ok;
  g.chain = sc->chain;
  HIPCHK(launch_gomp_relinearise(g, st));
  HIPCHK(hipEventRecord(sc->ev, st));
  HIPCHK(hipEventSynchronize(sc->ev));
  for (int j = 0; j < nq; j++) ok_out[j] = sc->h_ok[j];
  return MI_OSQP_OK;
}

// mi_gomp_scene_create (chain null: model 6 is refused as it always was), mi_gomp_scene_create_chain and
// mi_gomp_scene_create_world (capsules besides), mi_gomp_scene_create_cuboids (cuboids besides those) and
// mi_gomp_scene_create_pairs (ball pairs besides those), mi_gomp_scene_create_tilts (tilt limits besides those) and
// mi_gomp_scene_create_grids (distance grids besides those), mi_gomp_scene_create_goals (grasp goals besides those).
// Everything that can be refused is refused here on the host, the checks that need no handle first.
// every node of a grid is a finite number: the message names the first that is not, by its indices
static int gomp_grid_values_finite(const std::string &who, const int32_t *n, const double *values) {
  const size_t count = (size_t)n[0] * (size_t)n[1] * (size_t)n[2];
  for (size_t i = 0; i < count; i++)
    if (!std::isfinite(values[i])) {
      g_last_error = who + ": the value of node (" + std::to_string(i % (size_t)n[0]) + ", " + std::to_string(i / (size_t)n[0] % (size_t)n[1]) + ", " +
                     std::to_string(i / ((size_t)n[0] * (size_t)n[1])) + ") is not finite";
      return MI_OSQP_ERR_INVALID_DATA;
    }
  return 0;
}
// a goal scene re-linearises only QPs that have been told what they ask of the goals (ids out of range: cont_check_ids)
static int gomp_goal_values_set(const mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids) {
  if (!sc->n_goals) return 0;
  for (int64_t j = 0; j < n_ids; j++)
    if (ids[j] >= 0 && ids[j] < sc->h->B && !sc->goal_set[(size_t)ids[j]]) {
      g_last_error = "QP " + std::to_string(ids[j]) + ": the goal values were never set (mi_gomp_scene_set_goal_values)";
      return MI_OSQP_ERR_INVALID_DATA;
    }
  return 0;
}
static int gomp_scene_create(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain, bool chain_entry,
                             int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                             int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
                             int64_t n_pairs, const mi_gomp_pair *pairs, int64_t n_tilts, const mi_gomp_tilt *tilts,
                             int64_t n_grids, const mi_gomp_grid *grids, int64_t n_goals, const mi_gomp_goal *goals,
                             const double *con_lo, const double *con_hi) {
  if (!out) return MI_OSQP_ERR_NULL;
  *out = nullptr;
  if ((n_balls > 0 && !balls) || (n_lines > 0 && !lines)) return MI_OSQP_ERR_NULL;
  if (n_capsules > 0 && !capsules) { g_last_error = "n_capsules > 0 and no capsules"; return MI_OSQP_ERR_NULL; }
  if (n_capsules < 0) { g_last_error = "n_capsules is negative"; return MI_OSQP_ERR_INVALID_DATA; }
  for (int64_t c = 0; c < n_capsules; c++) {
    const mi_gomp_capsule &cp = capsules[c];
    bool finite = std::isfinite(cp.radius) && std::isfinite(cp.margin);
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(cp.a[k]) && std::isfinite(cp.b[k]);
    if (!finite) { g_last_error = "capsule " + std::to_string(c) + " has a field that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
    if (cp.radius < 0.0 || cp.margin < 0.0) { g_last_error = "capsule " + std::to_string(c) + ": radius and margin must not be negative"; return MI_OSQP_ERR_INVALID_DATA; }
  }
  if (n_cuboids > 0 && !cuboids) { g_last_error = "n_cuboids > 0 and no cuboids"; return MI_OSQP_ERR_NULL; }
  if (n_cuboids < 0) { g_last_error = "n_cuboids is negative"; return MI_OSQP_ERR_INVALID_DATA; }
  for (int64_t c = 0; c < n_cuboids; c++) {
    const mi_gomp_cuboid &cb = cuboids[c];
    bool finite = std::isfinite(cb.radius) && std::isfinite(cb.margin);
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(cb.centre[k]) && std::isfinite(cb.half[k]);
    for (int k = 0; k < 9; k++) finite = finite && std::isfinite(cb.axes[k]);
    if (!finite) { g_last_error = "cuboid " + std::to_string(c) + " has a field that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
    if (cb.half[0] < 0.0 || cb.half[1] < 0.0 || cb.half[2] < 0.0 || cb.radius < 0.0 || cb.margin < 0.0) {
      g_last_error = "cuboid " + std::to_string(c) + ": half extents, radius and margin must not be negative"; return MI_OSQP_ERR_INVALID_DATA;
    }
    for (int i = 0; i < 3; i++)
      for (int j = i; j < 3; j++) {
        const double dot = cb.axes[3 * i] * cb.axes[3 * j] + cb.axes[3 * i + 1] * cb.axes[3 * j + 1] + cb.axes[3 * i + 2] * cb.axes[3 * j + 2];
        if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-9)) { g_last_error = "cuboid " + std::to_string(c) + ": the axes are not orthonormal"; return MI_OSQP_ERR_INVALID_DATA; }
      }
  }
  if (n_pairs > 0 && !pairs) { g_last_error = "n_pairs > 0 and no pairs"; return MI_OSQP_ERR_NULL; }
  if (n_pairs < 0) { g_last_error = "n_pairs is negative"; return MI_OSQP_ERR_INVALID_DATA; }
  for (int64_t k = 0; k < n_pairs; k++) {
    const mi_gomp_pair &pr = pairs[k];
    if (!std::isfinite(pr.margin) || pr.margin < 0.0) { g_last_error = "pair " + std::to_string(k) + ": the margin must be finite and not negative"; return MI_OSQP_ERR_INVALID_DATA; }
    if (pr.a < 0 || pr.a >= n_balls || pr.b < 0 || pr.b >= n_balls) { g_last_error = "pair " + std::to_string(k) + ": a and b must be balls 0 .. n_balls - 1"; return MI_OSQP_ERR_INVALID_DATA; }
    if (pr.a == pr.b) { g_last_error = "pair " + std::to_string(k) + " joins a ball with itself"; return MI_OSQP_ERR_INVALID_DATA; }
    if (balls[pr.a].model == MI_GM_DH_CHAIN && balls[pr.b].model == MI_GM_DH_CHAIN && balls[pr.a].param[0] == balls[pr.b].param[0]) {
      g_last_error = "pair " + std::to_string(k) + " joins two chain balls of one frame: their distance is constant"; return MI_OSQP_ERR_INVALID_DATA;
    }
  }
  if (n_tilts > 0 && !tilts) { g_last_error = "n_tilts > 0 and no tilts"; return MI_OSQP_ERR_NULL; }
  if (n_tilts < 0) { g_last_error = "n_tilts is negative"; return MI_OSQP_ERR_INVALID_DATA; }
  if (n_tilts > 0 && !chain) { g_last_error = "tilt 0 names a frame of the chain and the scene has no chain"; return MI_OSQP_ERR_NULL; }
  GompChainDev hc{};
  if (chain_entry) {
    for (int64_t b = 0; b < n_balls; b++)
      if (balls[b].model == MI_GM_DH_CHAIN && !chain) { g_last_error = "ball " + std::to_string(b) + " is a chain ball and the scene has no chain"; return MI_OSQP_ERR_NULL; }
    if (chain) {
      const int nj = chain->n_joints;
      if (nj < 1 || nj > MI_GOMP_MAXD) { g_last_error = "chain: n_joints must be 1 .. 8"; return MI_OSQP_ERR_INVALID_DATA; }
      if (nj != dims) { g_last_error = "chain: n_joints differs from dims"; return MI_OSQP_ERR_INVALID_DATA; }
      for (int i = 0; i < nj; i++)
        if (!std::isfinite(chain->a[i]) || !std::isfinite(chain->d[i]) || !std::isfinite(chain->alpha[i]) || !std::isfinite(chain->theta0[i])) {
          g_last_error = "chain: joint " + std::to_string(i) + " has a parameter that is not finite"; return MI_OSQP_ERR_INVALID_DATA;
        }
      for (int64_t b = 0; b < n_balls; b++) {
        if (balls[b].model != MI_GM_DH_CHAIN) continue;
        const double *pm = balls[b].param;
        if (!std::isfinite(balls[b].radius) || !std::isfinite(pm[0]) || !std::isfinite(pm[1]) || !std::isfinite(pm[2]) || !std::isfinite(pm[3])) {
          g_last_error = "chain ball " + std::to_string(b) + " has a parameter that is not finite"; return MI_OSQP_ERR_INVALID_DATA;
        }
        if (pm[0] != std::floor(pm[0]) || pm[0] < 1.0 || pm[0] > (double)nj) { g_last_error = "chain ball " + std::to_string(b) + ": param[0] must be a frame 1 .. n_joints"; return MI_OSQP_ERR_INVALID_DATA; }
      }
      hc.n_joints = nj;
      for (int i = 0; i < nj; i++) { hc.a[i] = chain->a[i]; hc.d[i] = chain->d[i]; hc.ca[i] = std::cos(chain->alpha[i]); hc.sa[i] = std::sin(chain->alpha[i]); hc.theta0[i] = chain->theta0[i]; }
      for (int i = nj; i < MI_GOMP_MAXD; i++) hc.ca[i] = 1.0;      // (never part of a result: identity joints)
    }
  }
  // a tilt limit: the three cosines the kernel compares with are taken here, once, in fp64
  std::vector<GompTiltDev> htilt((size_t)(n_tilts > 0 ? n_tilts : 0));
  for (int64_t k = 0; k < n_tilts; k++) {
    const mi_gomp_tilt &tl = tilts[k];
    const std::string who = "tilt " + std::to_string(k);
    bool finite = std::isfinite(tl.max_angle) && std::isfinite(tl.margin);
    for (int i = 0; i < 3; i++) finite = finite && std::isfinite(tl.axis[i]) && std::isfinite(tl.ref[i]);
    if (!finite) { g_last_error = who + " has a field that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
    if (tl.frame < 1 || tl.frame > hc.n_joints) { g_last_error = who + ": frame must be 1 .. n_joints"; return MI_OSQP_ERR_INVALID_DATA; }
    const double na = std::sqrt(tl.axis[0] * tl.axis[0] + tl.axis[1] * tl.axis[1] + tl.axis[2] * tl.axis[2]);
    const double nr = std::sqrt(tl.ref[0] * tl.ref[0] + tl.ref[1] * tl.ref[1] + tl.ref[2] * tl.ref[2]);
    if (!(std::fabs(na - 1.0) <= 1e-9)) { g_last_error = who + ": axis is not a unit vector"; return MI_OSQP_ERR_INVALID_DATA; }
    if (!(std::fabs(nr - 1.0) <= 1e-9)) { g_last_error = who + ": ref is not a unit vector"; return MI_OSQP_ERR_INVALID_DATA; }
    if (!(tl.max_angle > 0.0 && tl.max_angle < M_PI)) { g_last_error = who + ": max_angle must lie in (0, pi)"; return MI_OSQP_ERR_INVALID_DATA; }
    if (tl.margin < 0.0) { g_last_error = who + ": the margin must not be negative"; return MI_OSQP_ERR_INVALID_DATA; }
    GompTiltDev &d = htilt[(size_t)k];
    d.frame = tl.frame; d.pad = 0;
    for (int i = 0; i < 3; i++) { d.axis[i] = tl.axis[i]; d.ref[i] = tl.ref[i]; }
    d.cos_lim = std::cos(tl.max_angle);
    d.cos_act = std::cos(std::max(0.0, tl.max_angle - tl.margin));
    d.cos_ok = std::cos(std::min(M_PI, tl.max_angle + 1e-3));
  }
  // a distance grid: shape, spacing and every node are checked here; 1 / cell is taken once, in fp64
  if (n_grids > 0 && !grids) { g_last_error = "n_grids > 0 and no grids"; return MI_OSQP_ERR_NULL; }
  if (n_grids < 0) { g_last_error = "n_grids is negative"; return MI_OSQP_ERR_INVALID_DATA; }
  std::vector<GompGridDev> hgrid((size_t)(n_grids > 0 ? n_grids : 0));
  std::vector<size_t> grid_off, grid_len;
  size_t grid_total = 0;
  for (int64_t k = 0; k < n_grids; k++) {
    const mi_gomp_grid &gr = grids[k];
    const std::string who = "grid " + std::to_string(k);
    if (!gr.values) { g_last_error = who + " has no values"; return MI_OSQP_ERR_NULL; }
    size_t count = 1;
    for (int i = 0; i < 3; i++) {
      if (gr.n[i] < 2 || gr.n[i] > 1024) { g_last_error = who + ": n[" + std::to_string(i) + "] must be 2 .. 1024"; return MI_OSQP_ERR_INVALID_DATA; }
      count *= (size_t)gr.n[i];
    }
    if (count > ((size_t)1 << 24)) { g_last_error = who + " has more than 2^24 values"; return MI_OSQP_ERR_INVALID_DATA; }
    if (!std::isfinite(gr.cell) || !std::isfinite(gr.offset) || !std::isfinite(gr.margin)) { g_last_error = who + " has a field that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
    for (int i = 0; i < 3; i++)
      if (!std::isfinite(gr.origin[i])) { g_last_error = who + " has an origin that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
    if (!(gr.cell > 0.0)) { g_last_error = who + ": cell must be positive"; return MI_OSQP_ERR_INVALID_DATA; }
    if (gr.offset < 0.0 || gr.margin < 0.0) { g_last_error = who + ": offset and margin must not be negative"; return MI_OSQP_ERR_INVALID_DATA; }
    if (int rc = gomp_grid_values_finite(who, gr.n, gr.values)) return rc;
    GompGridDev &d = hgrid[(size_t)k];
    for (int i = 0; i < 3; i++) { d.origin[i] = gr.origin[i]; d.n[i] = gr.n[i]; }
    d.inv_cell = 1.0 / gr.cell;
    d.sy = gr.n[0]; d.sz = gr.n[0] * gr.n[1]; d.pad = 0;
    d.offset = gr.offset; d.margin = gr.margin; d.values = nullptr;
    grid_off.push_back(grid_total); grid_len.push_back(count);
    grid_total += count;
  }
  // a grasp goal: the structure only; what each QP asks of it comes with mi_gomp_scene_set_goal_values
  if (n_goals > 0 && !goals) { g_last_error = "n_goals > 0 and no goals"; return MI_OSQP_ERR_NULL; }
  if (n_goals < 0 || n_goals > 4) { g_last_error = "n_goals must be 0 .. 4"; return MI_OSQP_ERR_INVALID_DATA; }
  std::vector<GompGoalDev> hgoal((size_t)n_goals);
  for (int64_t k = 0; k < n_goals; k++) {
    const mi_gomp_goal &gl = goals[k];
    const std::string who = "goal " + std::to_string(k);
    if (gl.ball < 0 || gl.ball >= n_balls) { g_last_error = who + ": ball must be 0 .. n_balls - 1"; return MI_OSQP_ERR_INVALID_DATA; }
    if (gl.waypoint < 0 || gl.waypoint >= waypoints) { g_last_error = who + ": waypoint must be 0 .. waypoints - 1"; return MI_OSQP_ERR_INVALID_DATA; }
    if (gl.frame >= 1 && !chain) { g_last_error = who + " names a frame of the chain and the scene has no chain"; return MI_OSQP_ERR_NULL; }
    if (gl.frame < 0 || gl.frame > hc.n_joints) { g_last_error = who + ": frame must be 0 .. n_joints"; return MI_OSQP_ERR_INVALID_DATA; }
    if (!(std::isfinite(gl.axis[0]) && std::isfinite(gl.axis[1]) && std::isfinite(gl.axis[2]))) { g_last_error = who + " has an axis that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
    const double na = std::sqrt(gl.axis[0] * gl.axis[0] + gl.axis[1] * gl.axis[1] + gl.axis[2] * gl.axis[2]);
    if (gl.frame >= 1 && !(std::fabs(na - 1.0) <= 1e-9)) { g_last_error = who + ": axis is not a unit vector"; return MI_OSQP_ERR_INVALID_DATA; }
    GompGoalDev &d = hgoal[(size_t)k];
    d.ball = gl.ball; d.waypoint = gl.waypoint; d.frame = gl.frame; d.pad = 0;
    for (int i = 0; i < 3; i++) d.axis[i] = gl.axis[i];
  }
  if (!h) return MI_OSQP_ERR_NULL;
  const Analysis &an = (*h->anp);
  const int D = (int)dims, W = (int)waypoints;
  if (D < 1 || D > 8 || W < 2 || n_balls < 0 || n_lines < 0 || an.n != 2 * D * W) return MI_OSQP_ERR_INVALID_DATA;
  // rows of the reference's layout ([REF] constraint-builder.h:34-44): links, position / velocity / acceleration boxes, then
  // D W (3 + |lines| |balls|) rows for the 3-D part, of which the populated ones come first
  const int row0 = (W - 1) * D + D * (W + W - 1 + W - 2);
  int rows3d = 0;
  for (int b = 0; b < (int)n_balls; b++) {
    if (balls[b].model < MI_GM_UR5E_FLANGE || balls[b].model > (hc.n_joints ? MI_GM_DH_CHAIN : MI_GM_TABLE)) return MI_OSQP_ERR_INVALID_DATA;
    if ((balls[b].model <= MI_GM_UR5E_ELBOW && D != 6) || ((balls[b].model == MI_GM_YAW_2LINK || balls[b].model == MI_GM_TABLE) && D != 3)) return MI_OSQP_ERR_INVALID_DATA;
    rows3d += W * ((balls[b].is_gripper ? 3 : 0) + (int)n_lines + (int)n_capsules + (int)n_cuboids + (int)n_grids);
  }
  const int pair_row0 = row0 + rows3d;                             // the pair rows: behind the block of the last ball, pair-major
  rows3d += W * (int)n_pairs;
  const int tilt_row0 = row0 + rows3d;                             // the tilt rows: behind the pair rows, tilt-major
  rows3d += W * (int)n_tilts;
  const int goal_row0 = row0 + rows3d;                             // the goal rows: behind the tilt rows, goal-major, four a goal
  rows3d += 4 * (int)n_goals;
  if (row0 + rows3d > an.m) {
    g_last_error = "the constraint matrix does not hold the 3-D rows of this scene";
    if (n_goals > 0 && goal_row0 <= an.m) g_last_error += " (goal " + std::to_string((an.m - goal_row0) / 4) + ")";   // the first goal without its rows
    else if (n_tilts > 0 && tilt_row0 <= an.m) g_last_error += " (tilt " + std::to_string((an.m - tilt_row0) / W) + ")";   // the first tilt without its rows
    else if (n_grids > 0) {                                        // the first grid row the matrix lacks, if a grid row is the first
      int r = row0;
      for (int b = 0; b < (int)n_balls && r <= an.m; b++)
        for (int w = 0; w < W && r <= an.m; w++) {
          const int before = (balls[b].is_gripper ? 3 : 0) + (int)n_lines + (int)n_capsules + (int)n_cuboids;
          if (an.m >= r + before && an.m < r + before + (int)n_grids) g_last_error += " (grid " + std::to_string(an.m - r - before) + ")";
          r += before + (int)n_grids;
        }
    }
    return MI_OSQP_ERR_INVALID_DATA;
  }
  DevGuard guard(h->device);
  mi_gomp_scene *sc = new (std::nothrow) mi_gomp_scene();
  if (!sc) return MI_OSQP_ERR_ALLOC;
  std::unique_ptr<mi_gomp_scene> own(sc);
  sc->h = h; sc->dims = D; sc->W = W; sc->n_balls = (int)n_balls; sc->n_lines = (int)n_lines; sc->n_caps = (int)n_capsules; sc->n_cuboids = (int)n_cuboids; sc->n_pairs = (int)n_pairs; sc->pair_row0 = pair_row0; sc->n_tilts = (int)n_tilts; sc->tilt_row0 = tilt_row0; sc->row0 = row0; sc->n_rows3d = rows3d; sc->n_grids = (int)n_grids; sc->n_goals = (int)n_goals; sc->goal_row0 = goal_row0;
  sc->chain = hc;
  for (int k = 0; k < 3; k++) { sc->con_lo[k] = con_lo ? con_lo[k] : -1e30; sc->con_hi[k] = con_hi ? con_hi[k] : 1e30; }
  // where the entries of the 3-D rows sit in A's value array: row r of waypoint w holds D entries in the columns of q_w
  std::vector<int> aidx((size_t)rows3d * D, -1);
  {
    int r = row0;
    auto locate = [&](int w) {                                     // row r of waypoint w: its D entries, false when A lacks one
      for (int j = 0; j < D; j++) {
        const int col = w * D + j;
        const int *lo = an.Ai.data() + an.Ap[col], *hi = an.Ai.data() + an.Ap[col + 1];
        const int *it = std::lower_bound(lo, hi, r);
        if (it == hi || *it != r) return false;
        aidx[(size_t)(r - row0) * D + j] = (int)(it - an.Ai.data());
      }
      return true;
    };
    for (int b = 0; b < (int)n_balls; b++)
      for (int w = 0; w < W; w++)
        for (int k = 0, before = (balls[b].is_gripper ? 3 : 0) + (int)n_lines + (int)n_capsules + (int)n_cuboids; k < before + (int)n_grids; k++, r++)
          if (!locate(w)) {
            g_last_error = "the constraint matrix does not hold the 3-D rows of this scene";
            if (k >= before) g_last_error += " (grid " + std::to_string(k - before) + ")";
            return MI_OSQP_ERR_INVALID_DATA;
          }
    for (int k = 0; k < (int)n_pairs; k++)
      for (int w = 0; w < W; w++, r++)
        if (!locate(w)) { g_last_error = "the constraint matrix does not hold the 3-D rows of this scene (pair " + std::to_string(k) + ")"; return MI_OSQP_ERR_INVALID_DATA; }
    for (int k = 0; k < (int)n_tilts; k++)
      for (int w = 0; w < W; w++, r++)
        if (!locate(w)) { g_last_error = "the constraint matrix does not hold the 3-D rows of this scene (tilt " + std::to_string(k) + ")"; return MI_OSQP_ERR_INVALID_DATA; }
    for (int k = 0; k < (int)n_goals; k++)
      for (int i = 0; i < 4; i++, r++)
        if (!locate(goals[k].waypoint)) { g_last_error = "the constraint matrix does not hold the 3-D rows of this scene (goal " + std::to_string(k) + ")"; return MI_OSQP_ERR_INVALID_DATA; }
  }
  std::vector<GompBallDev> hb((size_t)n_balls);
  for (int b = 0; b < (int)n_balls; b++) { hb[b].model = balls[b].model; hb[b].is_gripper = balls[b].is_gripper; hb[b].radius = balls[b].radius; for (int k = 0; k < 12; k++) hb[b].param[k] = balls[b].param[k]; }
  std::vector<GompLineDev> hl((size_t)n_lines);
  for (int li = 0; li < (int)n_lines; li++) {
    const double nrm = std::hypot(lines[li].dir[0], lines[li].dir[1]);
    if (!(nrm > 0.0)) return MI_OSQP_ERR_INVALID_DATA;
    hl[li].D[0] = lines[li].dir[0] / nrm; hl[li].D[1] = lines[li].dir[1] / nrm; hl[li].D[2] = 0.0;
    for (int k = 0; k < 3; k++) hl[li].A[k] = lines[li].point[k];
    hl[li].below = lines[li].below; hl[li].pad = 0;
  }
  std::vector<GompCapsuleDev> hcap((size_t)n_capsules);
  for (int c = 0; c < (int)n_capsules; c++) {
    GompCapsuleDev &d = hcap[c];
    for (int k = 0; k < 3; k++) { d.a[k] = capsules[c].a[k]; d.e[k] = capsules[c].b[k] - capsules[c].a[k]; }
    d.ee = d.e[0] * d.e[0] + d.e[1] * d.e[1] + d.e[2] * d.e[2];
    d.R = capsules[c].radius; d.margin = capsules[c].margin;
  }
  std::vector<GompCuboidDev> hcub((size_t)n_cuboids);
  for (int c = 0; c < (int)n_cuboids; c++) {
    GompCuboidDev &d = hcub[c];
    for (int k = 0; k < 3; k++) { d.o[k] = cuboids[c].centre[k]; d.h[k] = cuboids[c].half[k]; }
    for (int k = 0; k < 9; k++) d.u[k] = cuboids[c].axes[k];
    d.R = cuboids[c].radius; d.margin = cuboids[c].margin;
  }
  std::vector<GompPairDev> hpair((size_t)n_pairs);
  for (int k = 0; k < (int)n_pairs; k++) { hpair[k].a = pairs[k].a; hpair[k].b = pairs[k].b; hpair[k].margin = pairs[k].margin; }
  int rc;
  if ((rc = sc->balls.upload(hb)) || (rc = sc->lines.upload(hl)) || (n_capsules && (rc = sc->caps.upload(hcap))) || (n_cuboids && (rc = sc->cuboids.upload(hcub))) || (n_pairs && (rc = sc->pairs.upload(hpair))) || (n_tilts && (rc = sc->tilts.upload(htilt))) ||
      (rc = sc->aidx.upload(aidx)) ||
      (rc = sc->A.alloc((size_t)h->B * std::max(an.Ap[an.n], 1))) || (rc = sc->l.alloc((size_t)h->B * std::max(an.m, 1))) || (rc = sc->u.alloc((size_t)h->B * std::max(an.m, 1)))) return rc;
  if (n_grids > 0) {                                               // all nodes in one buffer, the descriptors (pointing into it) in a second
    if ((rc = sc->grid_vals.alloc(grid_total))) return rc;
    for (int k = 0; k < (int)n_grids; k++) {
      hgrid[k].values = sc->grid_vals.p + grid_off[k];
      HIPCHK(hipMemcpy(sc->grid_vals.p + grid_off[k], grids[k].values, grid_len[k] * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = sc->grids.upload(hgrid))) return rc;
    sc->grid_off = grid_off; sc->grid_len = grid_len;
  }
  if (n_goals > 0) {
    if ((rc = sc->goals.upload(hgoal)) || (rc = sc->goal_vals.alloc((size_t)h->B * (size_t)n_goals))) return rc;
    for (int k = 0; k < (int)n_goals; k++) sc->goal_frame.push_back(goals[k].frame);
    sc->goal_set.assign((size_t)h->B, 0);
  }
  HIPCHK(hostpool::alloc((void **)&sc->h_ok, (size_t)h->B * sizeof(int), &sc->h_ok_cap));
  HIPCHK(hipEventCreateWithFlags(&sc->ev, hipEventDisableTiming));
  if (h->cont.keepA) { g_last_error = "the solver already has a scene"; return MI_OSQP_ERR_INVALID_DATA; }
  h->cont.keepA = sc->A.p; h->cont.keepl = sc->l.p; h->cont.keepu = sc->u.p;
  *out = own.release();
  return MI_OSQP_OK;
}

extern "C" {

int mi_gomp_scene_create(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, int64_t n_balls, const mi_gomp_ball *balls,
                         int64_t n_lines, const mi_gomp_line *lines, const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, nullptr, false, n_balls, balls, n_lines, lines, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_chain(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                               int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines, const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, chain, true, n_balls, balls, n_lines, lines, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_world(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                               int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                               int64_t n_capsules, const mi_gomp_capsule *capsules, const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, chain, chain != nullptr, n_balls, balls, n_lines, lines, n_capsules, capsules, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_cuboids(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                                 int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                                 int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
                                 const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, chain, chain != nullptr, n_balls, balls, n_lines, lines, n_capsules, capsules, n_cuboids, cuboids, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_pairs(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                               int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                               int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
                               int64_t n_pairs, const mi_gomp_pair *pairs, const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, chain, chain != nullptr, n_balls, balls, n_lines, lines, n_capsules, capsules, n_cuboids, cuboids,
                           n_pairs, pairs, 0, nullptr, 0, nullptr, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_tilts(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                               int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                               int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
                               int64_t n_pairs, const mi_gomp_pair *pairs, int64_t n_tilts, const mi_gomp_tilt *tilts,
                               const double *con_lo, const double *con_hi) {
  return mi_gomp_scene_create_grids(out, h, dims, waypoints, chain, n_balls, balls, n_lines, lines, n_capsules, capsules, n_cuboids, cuboids,
                                    n_pairs, pairs, n_tilts, tilts, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_grids(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                               int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                               int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
                               int64_t n_pairs, const mi_gomp_pair *pairs, int64_t n_tilts, const mi_gomp_tilt *tilts,
                               int64_t n_grids, const mi_gomp_grid *grids, const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, chain, chain != nullptr, n_balls, balls, n_lines, lines, n_capsules, capsules, n_cuboids, cuboids,
                           n_pairs, pairs, n_tilts, tilts, n_grids, grids, 0, nullptr, con_lo, con_hi);
}
int mi_gomp_scene_create_goals(mi_gomp_scene **out, mi_osqp_batch *h, int64_t dims, int64_t waypoints, const mi_gomp_chain *chain,
                               int64_t n_balls, const mi_gomp_ball *balls, int64_t n_lines, const mi_gomp_line *lines,
                               int64_t n_capsules, const mi_gomp_capsule *capsules, int64_t n_cuboids, const mi_gomp_cuboid *cuboids,
                               int64_t n_pairs, const mi_gomp_pair *pairs, int64_t n_tilts, const mi_gomp_tilt *tilts,
                               int64_t n_grids, const mi_gomp_grid *grids, int64_t n_goals, const mi_gomp_goal *goals,
                               const double *con_lo, const double *con_hi) {
  return gomp_scene_create(out, h, dims, waypoints, chain, chain != nullptr, n_balls, balls, n_lines, lines, n_capsules, capsules, n_cuboids, cuboids,
                           n_pairs, pairs, n_tilts, tilts, n_grids, grids, n_goals, goals, con_lo, con_hi);
}
// what the listed QPs ask of the scene's goals: checked on the host, the cosines taken here in fp64, copied on the handle's
// stream; kept rows are not touched (the next assemble / re-linearisation of such a QP reads the new values)
int mi_gomp_scene_set_goal_values(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const mi_gomp_goal_value *values) {
  if (!sc || (n_ids > 0 && (!ids || !values))) return MI_OSQP_ERR_NULL;
  if (sc->n_goals == 0) { g_last_error = "the scene has no goals"; return MI_OSQP_ERR_INVALID_DATA; }
  if (n_ids < 0) { g_last_error = "n_ids is negative"; return MI_OSQP_ERR_INVALID_DATA; }
  mi_osqp_batch *h = sc->h;
  const size_t NG = (size_t)sc->n_goals;
  std::vector<GompGoalValDev> hv((size_t)n_ids * NG);
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) { g_last_error = "id " + std::to_string(ids[j]) + ": the handle has QPs 0 .. " + std::to_string(h->B - 1); return MI_OSQP_ERR_INVALID_DATA; }
    for (size_t k = 0; k < NG; k++) {
      const mi_gomp_goal_value &v = values[(size_t)j * NG + k];
      const std::string who = "goal " + std::to_string(k) + " of QP " + std::to_string(ids[j]);
      bool finite = std::isfinite(v.max_angle);
      for (int i = 0; i < 3; i++) finite = finite && std::isfinite(v.point[i]) && std::isfinite(v.tol[i]) && std::isfinite(v.ref[i]);
      if (!finite) { g_last_error = who + " has a value that is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
      if (v.tol[0] < 0.0 || v.tol[1] < 0.0 || v.tol[2] < 0.0) { g_last_error = who + ": tol must not be negative"; return MI_OSQP_ERR_INVALID_DATA; }
      if (sc->goal_frame[k] >= 1) {
        const double nr = std::sqrt(v.ref[0] * v.ref[0] + v.ref[1] * v.ref[1] + v.ref[2] * v.ref[2]);
        if (!(std::fabs(nr - 1.0) <= 1e-9)) { g_last_error = who + ": ref is not a unit vector"; return MI_OSQP_ERR_INVALID_DATA; }
        if (!(v.max_angle > 0.0 && v.max_angle < M_PI)) { g_last_error = who + ": max_angle must lie in (0, pi)"; return MI_OSQP_ERR_INVALID_DATA; }
      }
      GompGoalValDev &d = hv[(size_t)j * NG + k];
      for (int i = 0; i < 3; i++) { d.point[i] = v.point[i]; d.tol[i] = v.tol[i]; d.ref[i] = v.ref[i]; }
      d.cos_lim = std::cos(v.max_angle);
      d.cos_ok = std::cos(std::min(M_PI, v.max_angle + 1e-3));
    }
  }
  if (!n_ids) return MI_OSQP_OK;
  DevGuard guard(h->device);
  for (int64_t j = 0; j < n_ids; j++)
    HIPCHK(hipMemcpyAsync(sc->goal_vals.p + (size_t)ids[j] * NG, hv.data() + (size_t)j * NG, NG * sizeof(GompGoalValDev), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));          // (the staging array is pageable)
  for (int64_t j = 0; j < n_ids; j++) sc->goal_set[(size_t)ids[j]] = 1;
  return MI_OSQP_OK;
}
// a new camera frame: new node values of the same shape for grid k, on the handle's stream; kept rows are not touched
int mi_gomp_scene_update_grid(mi_gomp_scene *sc, int64_t k, const double *values) {
  if (!sc || !values) return MI_OSQP_ERR_NULL;
  if (sc->n_grids == 0) { g_last_error = "the scene has no grids"; return MI_OSQP_ERR_INVALID_DATA; }
  if (k < 0 || k >= sc->n_grids) { g_last_error = "grid " + std::to_string(k) + ": the scene has grids 0 .. " + std::to_string(sc->n_grids - 1); return MI_OSQP_ERR_INVALID_DATA; }
  for (size_t i = 0; i < sc->grid_len[(size_t)k]; i++)
    if (!std::isfinite(values[i])) { g_last_error = "grid " + std::to_string(k) + ": value " + std::to_string(i) + " is not finite"; return MI_OSQP_ERR_INVALID_DATA; }
  mi_osqp_batch *h = sc->h;
  DevGuard guard(h->device);
  HIPCHK(hipMemcpyAsync(sc->grid_vals.p + sc->grid_off[(size_t)k], values, sc->grid_len[(size_t)k] * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));          // (the caller's array is pageable)
  return MI_OSQP_OK;
}

void mi_gomp_scene_free(mi_gomp_scene *sc) {
  if (!sc) return;
  DevGuard guard(sc->h->device);
  (void)hipStreamSynchronize(sc->h->stream);
  if (sc->h->cont.keepA == sc->A.p) sc->h->cont.keepA = sc->h->cont.keepl = sc->h->cont.keepu = nullptr;
  delete sc;
}

// the raw constraint data of the listed QPs as the host built them (ConstraintBuilder::build): kept on the device
int mi_gomp_scene_set_rows(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *Av, const double *l, const double *u) {
  if (!sc || (n_ids > 0 && (!ids || !Av || !l || !u))) return MI_OSQP_ERR_NULL;
  mi_osqp_batch *h = sc->h;
  DevGuard guard(h->device);
  const Analysis &an = (*h->anp);
  const size_t nnzA = (size_t)an.Ap[an.n], m = (size_t)an.m;
  hipStream_t st = h->stream;
  for (int64_t j = 0; j < n_ids; j++) {
    if (ids[j] < 0 || ids[j] >= h->B) return MI_OSQP_ERR_INVALID_DATA;
    HIPCHK(hipMemcpyAsync(sc->A.p + (size_t)ids[j] * nnzA, Av + (size_t)j * nnzA, nnzA * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sc->l.p + (size_t)ids[j] * m, l + (size_t)j * m, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sc->u.p + (size_t)ids[j] * m, u + (size_t)j * m, m * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));          // (the caller's arrays are pageable)
  return MI_OSQP_OK;
}
int mi_gomp_scene_get_rows(mi_gomp_scene *sc, int64_t id, double *Av, double *l, double *u) {
  if (!sc) return MI_OSQP_ERR_NULL;
  mi_osqp_batch *h = sc->h;
  if (id < 0 || id >= h->B) return MI_OSQP_ERR_INVALID_DATA;
  DevGuard guard(h->device);
  const Analysis &an = (*h->anp);
  const size_t nnzA = (size_t)an.Ap[an.n], m = (size_t)an.m;
  if (Av) HIPCHK(hipMemcpy(Av, sc->A.p + (size_t)id * nnzA, nnzA * sizeof(double), hipMemcpyDeviceToHost));
  if (l) HIPCHK(hipMemcpy(l, sc->l.p + (size_t)id * m, m * sizeof(double), hipMemcpyDeviceToHost));
  if (u) HIPCHK(hipMemcpy(u, sc->u.p + (size_t)id * m, m * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OSQP_OK;
}

// withObstacles(con_3d, x) for the listed QPs' kept rows, without touching the solver (tests; the first linearisation of a segment)
int mi_gomp_assemble_some(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *x, int32_t *ok_out) {
  if (!sc || (n_ids > 0 && (!ids || !x || !ok_out))) return MI_OSQP_ERR_NULL;
  if (!n_ids) return MI_OSQP_OK;
  if (int rg = gomp_goal_values_set(sc, n_ids, ids)) return rg;
  DevGuard guard(sc->h->device);
  int rc;
  if ((rc = cont_enter(sc->h)) || (rc = cont_check_ids(sc->h, n_ids, ids, false))) return rc;
  return gomp_launch(sc, n_ids, ids, x, 1, ok_out);
}

// One SQP step of the listed (finished) QPs on the device: isSolutionOK of their solutions x; the QPs whose trajectory is not
// acceptable are re-linearised around it (their kept 3-D rows rewritten) and updated (= builder.withObstacles(con_3d, x) +
// QPSolver::update, [REF] src/gomp-solver.h:79-87) - they are ready for solve_begin_some.  ok_out[j] = 1: trajectory accepted.
int mi_gomp_relinearise_some(mi_gomp_scene *sc, int64_t n_ids, const int64_t *ids, const double *x, int32_t *ok_out) {
  CallTimer timer_("gomp_relinearise_some");
  if (!sc || (n_ids > 0 && (!ids || !x || !ok_out))) return MI_OSQP_ERR_NULL;
  if (!n_ids) return MI_OSQP_OK;
  if (int rg = gomp_goal_values_set(sc, n_ids, ids)) return rg;
  mi_osqp_batch *h = sc->h;
  DevGuard guard(h->device);
  int rc;
  if ((rc = cont_enter(h)) || (rc = cont_check_ids(h, n_ids, ids, true))) return rc;
  // the acceptance test; the trajectories that fail it get new 3-D rows in the same launch (an accepted trajectory's rows
  // stay as they are: its solver is not updated) ...
  if ((rc = gomp_launch(sc, n_ids, ids, x, 2, ok_out))) return rc;
  std::vector<int64_t> bad;
  for (int64_t j = 0; j < n_ids; j++) if (!ok_out[j]) bad.push_back(ids[j]);
  if (bad.empty()) return MI_OSQP_OK;
  // ... and the update from the device-resident data
  return cont_new_data(h, (int64_t)bad.size(), bad.data(), nullptr, nullptr, nullptr, false, sc->A.p, sc->l.p, sc->u.p);
}

}  // extern "C"

extern "C" {

// ------------------------------------------------------------------ single QP

int mi_osqp_setup(mi_osqp_solver **out, int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi, const double *Pv,
                  const double *q, const int64_t *Ap, const int64_t *Ai, const double *Av, const double *l,
                  const double *u, const mi_osqp_settings *settings) {
  if (!out) return MI_OSQP_ERR_NULL;
  *out = nullptr;
  mi_osqp_batch *b = nullptr;
  int rc = mi_osqp_batch_setup(&b, 1, n, m, Pp, Pi, Pv, q, Ap, Ai, Av, l, u, settings, -1);
  if (rc) return rc;
  mi_osqp_solver *s = new (std::nothrow) mi_osqp_solver();
  if (!s) { delete b; return MI_OSQP_ERR_ALLOC; }
  s->b = b; *out = s;
  return MI_OSQP_OK;
}
void mi_osqp_free(mi_osqp_solver *h) { if (h) { delete h->b; delete h; } }
int mi_osqp_update_A_bounds(mi_osqp_solver *h, const int64_t *Ap, const int64_t *Ai, const double *Av, const double *l, const double *u) {
  return h ? mi_osqp_batch_update_A_bounds(h->b, Ap, Ai, Av, l, u) : MI_OSQP_ERR_NULL;
}
int mi_osqp_update_A(mi_osqp_solver *h, const int64_t *Ap, const int64_t *Ai, const double *Av) {
  return h ? mi_osqp_batch_update_A(h->b, Ap, Ai, Av) : MI_OSQP_ERR_NULL;
}
int mi_osqp_update_bounds(mi_osqp_solver *h, const double *l, const double *u) {
  return h ? mi_osqp_batch_update_bounds(h->b, l, u) : MI_OSQP_ERR_NULL;
}
int mi_osqp_warm_start_x(mi_osqp_solver *h, const double *x) { return h ? mi_osqp_batch_warm_start_x(h->b, x) : MI_OSQP_ERR_NULL; }
int mi_osqp_update_q(mi_osqp_solver *h, const double *q) { return h ? mi_osqp_batch_update_q(h->b, q) : MI_OSQP_ERR_NULL; }
int mi_osqp_update_P(mi_osqp_solver *h, const int64_t *Pp, const int64_t *Pi, const double *Pv) {
  return h ? mi_osqp_batch_update_P(h->b, Pp, Pi, Pv) : MI_OSQP_ERR_NULL;
}
int mi_osqp_update_P_A(mi_osqp_solver *h, const int64_t *Pp, const int64_t *Pi, const double *Pv, const int64_t *Ap, const int64_t *Ai,
                       const double *Av) {
  return h ? mi_osqp_batch_update_P_A(h->b, Pp, Pi, Pv, Ap, Ai, Av) : MI_OSQP_ERR_NULL;
}
int mi_osqp_warm_start_y(mi_osqp_solver *h, const double *y) { return h ? mi_osqp_batch_warm_start_y(h->b, y) : MI_OSQP_ERR_NULL; }
int mi_osqp_solve(mi_osqp_solver *h, mi_osqp_info *info) {
  if (!h) return MI_OSQP_ERR_NULL;
  int rc = mi_osqp_batch_solve(h->b);
  if (rc) return rc;
  if (info) return mi_osqp_batch_get_info(h->b, info);
  return MI_OSQP_OK;
}
int mi_osqp_get_primal(mi_osqp_solver *h, double *x) { return h ? mi_osqp_batch_get_primal(h->b, x) : MI_OSQP_ERR_NULL; }
int mi_osqp_get_dual(mi_osqp_solver *h, double *y) { return h ? mi_osqp_batch_get_dual(h->b, y) : MI_OSQP_ERR_NULL; }
int mi_osqp_get_prim_inf_cert(mi_osqp_solver *h, double *dy_out) { return h ? mi_osqp_batch_get_prim_inf_cert(h->b, dy_out) : MI_OSQP_ERR_NULL; }
int mi_osqp_get_dual_inf_cert(mi_osqp_solver *h, double *dx_out) { return h ? mi_osqp_batch_get_dual_inf_cert(h->b, dx_out) : MI_OSQP_ERR_NULL; }
int mi_osqp_adjoint(mi_osqp_solver *h, const double *dx, const double *dy, double *dq, double *dP, double *dA, double *dl, double *du,
                    int32_t *status) {
  return h ? mi_osqp_batch_adjoint(h->b, dx, dy, dq, dP, dA, dl, du, status) : MI_OSQP_ERR_NULL;
}
int mi_osqp_debug_refactor_chunks(int64_t n_flagged, const int64_t *flagged, int64_t n_active, const int64_t *active, int64_t tile,
                                  int64_t chunk_qps, int64_t max_chunks, int64_t *n_chunks, int64_t *work_begin, int64_t *tiles,
                                  int64_t *tile_begin) {
  if (!n_chunks || !work_begin || !tiles || !tile_begin || (n_flagged > 0 && !flagged) || (n_active > 0 && !active)) return MI_OSQP_ERR_NULL;
  if (n_flagged < 0 || n_active < 0 || tile < 1 || chunk_qps < 1 || max_chunks < 1) return MI_OSQP_ERR_INVALID_DATA;
  const std::vector<int> f(flagged, flagged + n_flagged), a(active, active + n_active);
  const RefactorChunks ch = refactor_chunks(f, a, (int)tile, (int)chunk_qps, (int)max_chunks);
  *n_chunks = ch.n_chunks;
  std::copy(ch.work_begin.begin(), ch.work_begin.end(), work_begin);
  std::copy(ch.tiles.begin(), ch.tiles.end(), tiles);
  std::copy(ch.tile_begin.begin(), ch.tile_begin.end(), tile_begin);
  return MI_OSQP_OK;
}
int mi_osqp_debug_region_chunks(int64_t nq, int64_t gw, int64_t n_cus, int64_t *chunk_qps, int64_t *n_chunks) {
  if (!chunk_qps || !n_chunks) return MI_OSQP_ERR_NULL;
  if (nq < 0 || nq > INT32_MAX || gw < 0 || gw > INT32_MAX || n_cus < 1 || n_cus > INT32_MAX) return MI_OSQP_ERR_INVALID_DATA;
  const int q = region_chunk_qps((int)nq, (int)gw, (int)n_cus, streampool::kPipeChunks);
  *chunk_qps = q; *n_chunks = (nq + q - 1) / q;
  return MI_OSQP_OK;
}
int mi_osqp_debug_refactor_lanes(int64_t n_flagged, const int64_t *flagged, int64_t n_active, const int64_t *active, int64_t tile,
                                 int64_t chunk_qps, int64_t max_chunks, int64_t kbt, int64_t lanes, int64_t chunk0_first,
                                 int64_t scratch_slots, int64_t *n_lanes, int64_t *lane_of, int64_t *order, int64_t *order_begin,
                                 int64_t *scratch_begin, int64_t *n_waits, int64_t *wait_chunk, int64_t *wait_for) {
  if (!n_lanes || !lane_of || !order || !order_begin || !scratch_begin || !n_waits || !wait_chunk || !wait_for ||
      (n_flagged > 0 && !flagged) || (n_active > 0 && !active)) return MI_OSQP_ERR_NULL;
  if (n_flagged < 0 || n_active < 0 || tile < 1 || chunk_qps < 1 || max_chunks < 1 || kbt < 1 || lanes < 1 || lanes > 3 || scratch_slots < 0)
    return MI_OSQP_ERR_INVALID_DATA;
  const std::vector<int> f(flagged, flagged + n_flagged), a(active, active + n_active);
  const RefactorChunks ch = refactor_chunks(f, a, (int)tile, (int)chunk_qps, (int)max_chunks);
  const RefactorLanes rl = refactor_lanes(ch, f, (int)tile, (int)kbt, (int)lanes, chunk0_first != 0, (int)std::min<int64_t>(scratch_slots, INT32_MAX));
  *n_lanes = rl.n_lanes;
  std::copy(rl.lane_of.begin(), rl.lane_of.end(), lane_of);
  order_begin[0] = 0;
  for (int l = 0; l < rl.n_lanes; l++) {
    std::copy(rl.order[l].begin(), rl.order[l].end(), order + order_begin[l]);
    order_begin[l + 1] = order_begin[l] + (int64_t)rl.order[l].size();
  }
  std::copy(rl.scratch_begin.begin(), rl.scratch_begin.begin() + ch.n_chunks, scratch_begin);
  *n_waits = (int64_t)rl.wait_chunk.size();
  std::copy(rl.wait_chunk.begin(), rl.wait_chunk.end(), wait_chunk);
  std::copy(rl.wait_for.begin(), rl.wait_for.end(), wait_for);
  return MI_OSQP_OK;
}
int mi_osqp_debug_runahead_group(int64_t n_active, const int64_t *tiles, const double *pri_res, const double *dua_res, int64_t size,
                                 int64_t min_active, int64_t *n_group, int64_t *group) {
  if (!n_group || !group || (n_active > 0 && (!tiles || !pri_res || !dua_res))) return MI_OSQP_ERR_NULL;
  if (n_active < 0 || n_active > INT32_MAX || size < 0 || size > INT32_MAX || min_active < 0 || min_active > INT32_MAX) return MI_OSQP_ERR_INVALID_DATA;
  std::vector<int> t((size_t)n_active);
  for (int64_t i = 0; i < n_active; i++) {
    if (tiles[i] < 0 || tiles[i] > INT32_MAX || pri_res[i] < 0.0 || dua_res[i] < 0.0) return MI_OSQP_ERR_INVALID_DATA;
    t[(size_t)i] = (int)tiles[i];
  }
  {
    std::vector<int> sorted = t;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return MI_OSQP_ERR_INVALID_DATA;
  }
  const std::vector<int> g = runahead_group(t, std::vector<double>(pri_res, pri_res + n_active), std::vector<double>(dua_res, dua_res + n_active),
                                            (int)size, (int)min_active);
  *n_group = (int64_t)g.size();
  std::copy(g.begin(), g.end(), group);
  return MI_OSQP_OK;
}
int mi_osqp_debug_iterate_form(int64_t tiles, int64_t has_head, int64_t forced_form, int64_t long_min, int64_t *form) {
  if (!form) return MI_OSQP_ERR_NULL;
  if (tiles < 0 || tiles > INT32_MAX || forced_form < 0 || forced_form > 2 || long_min < -1 || long_min > INT32_MAX)
    return MI_OSQP_ERR_INVALID_DATA;
  Tuning t;
  t.rf_form = (int)forced_form; t.rf_long_min = (int)long_min;
  *form = iterate_form((int)tiles, has_head != 0, t);
  return MI_OSQP_OK;
}
int mi_osqp_debug_index_words_fit(int64_t resident_state, int64_t lds_vector, int64_t tile, int64_t threads, int64_t n, int64_t m,
                                  int64_t *fit, int64_t *xloc_trips, int64_t *pinv_trips) {
  if (!fit || !xloc_trips || !pinv_trips) return MI_OSQP_ERR_NULL;
  if ((tile != 1 && tile != 2 && tile != 4) || threads < 64 || threads > 1024 || threads % 64 || n < 1 || m < 0 || n + m > (int64_t)1 << 30)
    return MI_OSQP_ERR_INVALID_DATA;
  *fit = index_words_fit(resident_state != 0, lds_vector != 0, (int)tile, (int)threads, n, m) ? 1 : 0;
  *xloc_trips = MI_IX_XLOC_TRIPS; *pinv_trips = MI_IX_PINV_TRIPS;
  return MI_OSQP_OK;
}
int mi_osqp_get_stats(mi_osqp_solver *h, mi_osqp_stats *st) { return h ? mi_osqp_batch_get_stats(h->b, st) : MI_OSQP_ERR_NULL; }
int mi_osqp_get_settings(mi_osqp_solver *h, mi_osqp_settings *out) { return h ? mi_osqp_batch_get_settings(h->b, out) : MI_OSQP_ERR_NULL; }
int mi_osqp_update_settings(mi_osqp_solver *h, const mi_osqp_settings *s) { return h ? mi_osqp_batch_update_settings(h->b, s) : MI_OSQP_ERR_NULL; }

// ------------------------------------------------------------ multi-GPU batch
// block partition of the batch over the devices, one host thread per shard, no data-path collective.

}  // extern "C"

// One long-lived worker thread per shard (a planner calls update / warm start / solve / get_* several times per SQP step:
// creating and joining a thread per shard and call cost ~0.1 ms of host time each).  A job is posted to every worker; the
// caller waits for all of them - or, for solve_async, comes back later (wait).
struct ShardWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<int()> job;
  bool has_job = false, busy = false, quit = false;
  int rc = 0;
  std::string err;
  void start() {
    th = std::thread([this] {
      std::unique_lock<std::mutex> lk(mu);
      for (;;) {
        cv.wait(lk, [this] { return has_job || quit; });
        if (quit) return;
        std::function<int()> f = std::move(job);
        has_job = false;
        lk.unlock();
        const int r = f();
        const std::string e = r ? g_last_error : std::string();
        lk.lock();
        rc = r; err = e; busy = false;
        cv.notify_all();
      }
    });
  }
  void post(std::function<int()> f) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !busy; });
    job = std::move(f); has_job = true; busy = true; rc = 0; err.clear();
    cv.notify_all();
  }
  int wait(std::string &e) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !busy; });
    e = err;
    return rc;
  }
  ~ShardWorker() {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
};

struct mi_osqp_multi {
  int64_t B = 0, n = 0, m = 0;
  std::vector<int64_t> dev, begin;                 // begin has one entry more than there are shards
  std::vector<mi_osqp_batch *> shard;
  std::vector<std::unique_ptr<ShardWorker>> worker;
  bool async_pending = false;                      // a solve_async whose wait() has not been called
  ~mi_osqp_multi() { worker.clear(); for (mi_osqp_batch *b : shard) delete b; }      // (the workers finish their jobs first)
  size_t count() const { return shard.size(); }
};

// wait for the jobs posted to the workers; first error wins, its text becomes this thread's last error
static int multi_join(mi_osqp_multi *h) {
  int rc = MI_OSQP_OK;
  for (size_t k = 0; k < h->worker.size(); k++) {
    std::string e;
    const int r = h->worker[k]->wait(e);
    if (r && !rc) { rc = r; g_last_error = "shard " + std::to_string(k) + ": " + e; }
  }
  h->async_pending = false;
  return rc;
}
// run fn(shard index) on the shard's worker thread and wait for all of them
template <class F>
static int multi_fan_out(mi_osqp_multi *h, F &&fn) {
  const size_t ns = h->count();
  if (h->async_pending) { const int rc0 = multi_join(h); if (rc0) return rc0; }
  if (ns == 1) { const int rc = fn(0); if (rc) g_last_error = "shard 0: " + g_last_error; return rc; }
  if (h->worker.size() != ns) {
    h->worker.clear();
    for (size_t k = 0; k < ns; k++) { h->worker.emplace_back(new ShardWorker()); h->worker.back()->start(); }
  }
  for (size_t k = 0; k < ns; k++) h->worker[k]->post([&fn, k]() -> int { return fn(k); });
  return multi_join(h);
}

extern "C" {

int mi_osqp_multi_batch_setup(mi_osqp_multi **out, int64_t n_devices, const int64_t *devices, int64_t B, int64_t n, int64_t m,
                              const int64_t *Pp, const int64_t *Pi, const double *Pv, const double *q, const int64_t *Ap,
                              const int64_t *Ai, const double *Av, const double *l, const double *u,
                              const mi_osqp_settings *settings) {
  if (!out) return MI_OSQP_ERR_NULL;
  *out = nullptr;
  if (n_devices <= 0 || B <= 0 || n <= 0 || m < 0 || !Pp || !Ap) return MI_OSQP_ERR_INVALID_DATA;
  if (n_devices > B) n_devices = B;                 // never an empty shard
  mi_osqp_multi *h = new (std::nothrow) mi_osqp_multi();
  if (!h) return MI_OSQP_ERR_ALLOC;
  h->B = B; h->n = n; h->m = m;
  const int64_t base = B / n_devices, rem = B % n_devices;
  h->begin.push_back(0);
  for (int64_t k = 0; k < n_devices; k++) {
    h->dev.push_back(devices ? devices[k] : k);
    h->begin.push_back(h->begin.back() + base + (k < rem ? 1 : 0));
  }
  h->shard.assign((size_t)n_devices, nullptr);
  const int64_t nnzP = Pp[n], nnzA = Ap[n];
  int rc = multi_fan_out(h, [&](size_t k) -> int {
    const int64_t b0 = h->begin[k], nb = h->begin[k + 1] - b0;
    return mi_osqp_batch_setup(&h->shard[k], nb, n, m, Pp, Pi, Pv ? Pv + b0 * nnzP : nullptr, q ? q + b0 * n : nullptr, Ap, Ai,
                               Av ? Av + b0 * nnzA : nullptr, l ? l + b0 * m : nullptr, u ? u + b0 * m : nullptr, settings, h->dev[k]);
  });
  if (rc) { delete h; return rc; }
  *out = h;
  return MI_OSQP_OK;
}

void mi_osqp_multi_batch_free(mi_osqp_multi *h) { delete h; }
int64_t mi_osqp_multi_batch_shards(mi_osqp_multi *h) { return h ? (int64_t)h->count() : 0; }
int mi_osqp_multi_batch_shard(mi_osqp_multi *h, int64_t k, int64_t *device, int64_t *begin, int64_t *end, mi_osqp_batch **handle) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (k < 0 || k >= (int64_t)h->count()) return MI_OSQP_ERR_INVALID_DATA;
  if (device) *device = h->shard[k]->device;
  if (begin) *begin = h->begin[k];
  if (end) *end = h->begin[k + 1];
  if (handle) *handle = h->shard[k];
  return MI_OSQP_OK;
}
int mi_osqp_multi_batch_update_A(mi_osqp_multi *h, const int64_t *Ap, const int64_t *Ai, const double *Av) {
  if (!h || !Ap || !Ai || !Av) return MI_OSQP_ERR_NULL;
  const int64_t nnzA = Ap[h->n];
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_update_A(h->shard[k], Ap, Ai, Av + h->begin[k] * nnzA); });
}
int mi_osqp_multi_batch_update_bounds(mi_osqp_multi *h, const double *l, const double *u) {
  if (!h || !l || !u) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_update_bounds(h->shard[k], l + h->begin[k] * h->m, u + h->begin[k] * h->m); });
}
int mi_osqp_multi_batch_update_A_bounds(mi_osqp_multi *h, const int64_t *Ap, const int64_t *Ai, const double *Av, const double *l, const double *u) {
  if (!h || !Ap || !Ai || !Av || !l || !u) return MI_OSQP_ERR_NULL;
  const int64_t nnzA = Ap[h->n];
  return multi_fan_out(h, [&](size_t k) {
    return mi_osqp_batch_update_A_bounds(h->shard[k], Ap, Ai, Av + h->begin[k] * nnzA, l + h->begin[k] * h->m, u + h->begin[k] * h->m);
  });
}
int mi_osqp_multi_batch_warm_start_x(mi_osqp_multi *h, const double *x) {
  if (!h || !x) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_warm_start_x(h->shard[k], x + h->begin[k] * h->n); });
}
int mi_osqp_multi_batch_update_q(mi_osqp_multi *h, const double *q) {
  if (!h || !q) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_update_q(h->shard[k], q + h->begin[k] * h->n); });
}
int mi_osqp_multi_batch_update_P(mi_osqp_multi *h, const int64_t *Pp, const int64_t *Pi, const double *Pv) {
  if (!h || !Pp || !Pi || !Pv) return MI_OSQP_ERR_NULL;
  const int64_t nnzP = Pp[h->n];
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_update_P(h->shard[k], Pp, Pi, Pv + h->begin[k] * nnzP); });
}
int mi_osqp_multi_batch_update_P_A(mi_osqp_multi *h, const int64_t *Pp, const int64_t *Pi, const double *Pv, const int64_t *Ap,
                                   const int64_t *Ai, const double *Av) {
  if (!h || !Pp || !Pi || !Pv || !Ap || !Ai || !Av) return MI_OSQP_ERR_NULL;
  const int64_t nnzP = Pp[h->n], nnzA = Ap[h->n];
  return multi_fan_out(h, [&](size_t k) {
    return mi_osqp_batch_update_P_A(h->shard[k], Pp, Pi, Pv + h->begin[k] * nnzP, Ap, Ai, Av + h->begin[k] * nnzA);
  });
}
int mi_osqp_multi_batch_warm_start_y(mi_osqp_multi *h, const double *y) {
  if (!h || !y) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_warm_start_y(h->shard[k], y + h->begin[k] * h->m); });
}
// settings updates: every shard holds the same settings, so shard 0 decides for all before any shard changes
int mi_osqp_multi_batch_get_settings(mi_osqp_multi *h, mi_osqp_settings *out) {
  if (!h || !out) return MI_OSQP_ERR_NULL;
  if (h->async_pending) { const int rc0 = multi_join(h); if (rc0) return rc0; }
  return mi_osqp_batch_get_settings(h->shard[0], out);
}
int mi_osqp_multi_batch_update_settings(mi_osqp_multi *h, const mi_osqp_settings *s) {
  if (!h || !s) return MI_OSQP_ERR_NULL;
  if (h->async_pending) { const int rc0 = multi_join(h); if (rc0) return rc0; }
  const mi_osqp_settings cur = from_settings(h->shard[0]->st);
  int rc;
  if ((rc = settings_update_decide(cur, *s))) return rc;
  if (s->adaptive_rho_interval == 0 && cur.adaptive_rho_interval != 0 && !h->shard[0]->rho_interval_auto) {
    g_last_error = "settings update: adaptive_rho_interval is fixed at setup (0 is accepted where setup derived it from 0)";
    return MI_OSQP_ERR_INVALID_SETTINGS;
  }
  return multi_fan_out(h, [&](size_t k) -> int {
    mi_osqp_batch *b = h->shard[k];
    DevGuard guard(b->device);
    const int rc_ = cont_leave(b);
    return rc_ ? rc_ : mi_osqp_batch_update_settings(b, s);
  });
}
int mi_osqp_multi_batch_update_rho_each(mi_osqp_multi *h, const double *rho) {
  if (!h || !rho) return MI_OSQP_ERR_NULL;
  const int rc = check_rho_values(h->B, rho);
  if (rc) return rc;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_update_rho_each(h->shard[k], rho + h->begin[k]); });
}
int mi_osqp_multi_batch_solve(mi_osqp_multi *h) {
  if (!h) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_solve(h->shard[k]); });
}
// solve on every shard without waiting: the call returns once the jobs are with the shard workers; wait() joins them and
// reports the first error.  Any other multi-batch call joins a pending solve first.
int mi_osqp_multi_batch_solve_async(mi_osqp_multi *h) {
  if (!h) return MI_OSQP_ERR_NULL;
  if (h->async_pending) { const int rc0 = multi_join(h); if (rc0) return rc0; }
  const size_t ns = h->count();
  if (h->worker.size() != ns) {
    h->worker.clear();
    for (size_t k = 0; k < ns; k++) { h->worker.emplace_back(new ShardWorker()); h->worker.back()->start(); }
  }
  for (size_t k = 0; k < ns; k++) { mi_osqp_batch *b = h->shard[k]; h->worker[k]->post([b]() -> int { return mi_osqp_batch_solve(b); }); }
  h->async_pending = true;
  return MI_OSQP_OK;
}
int mi_osqp_multi_batch_wait(mi_osqp_multi *h) {
  if (!h) return MI_OSQP_ERR_NULL;
  return h->async_pending ? multi_join(h) : (int)MI_OSQP_OK;
}
int mi_osqp_multi_batch_get_primal(mi_osqp_multi *h, double *x) {
  if (!h || !x) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_get_primal(h->shard[k], x + h->begin[k] * h->n); });
}
int mi_osqp_multi_batch_get_dual(mi_osqp_multi *h, double *y) {
  if (!h || !y) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_get_dual(h->shard[k], y + h->begin[k] * h->m); });
}
int mi_osqp_multi_batch_get_prim_inf_cert(mi_osqp_multi *h, double *dy_out) {
  if (!h || !dy_out) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_get_prim_inf_cert(h->shard[k], dy_out + h->begin[k] * h->m); });
}
int mi_osqp_multi_batch_get_dual_inf_cert(mi_osqp_multi *h, double *dx_out) {
  if (!h || !dx_out) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_get_dual_inf_cert(h->shard[k], dx_out + h->begin[k] * h->n); });
}
int mi_osqp_multi_batch_get_info(mi_osqp_multi *h, mi_osqp_info *info) {
  if (!h || !info) return MI_OSQP_ERR_NULL;
  return multi_fan_out(h, [&](size_t k) { return mi_osqp_batch_get_info(h->shard[k], info + h->begin[k]); });
}

// ------------------------------------------------------ host-only diagnostics

int mi_osqp_debug_host_kkt_solve(int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi, const double *Pv,
                                 const int64_t *Ap, const int64_t *Ai, const double *Av, const double *l,
                                 const double *u, const mi_osqp_settings *settings, int64_t tile, const double *rhs,
                                 double *sol_schedule, double *sol_direct, mi_osqp_stats *st) {
  Settings s = to_settings(settings);
  if (validate_settings(s)) return MI_OSQP_ERR_INVALID_SETTINGS;
  Analysis an;
  // tile > 1: the dataflow form for tile - 1 workgroups per QP (global solve vector, no dense tail)
  const Tuning tu = tuning_from_env();
  const AnalysisTuning tune = tu.analysis;
  const int nwaves = tu.threads ? tu.threads / 64 : 8;      // (MI_OSQP_THREADS: the schedules of that many waves per tile)
  int rc = tile > 1 ? analyze(n, m, Pp, Pi, Ap, Ai, tune, an, 8, 1, -1, 0, (int)tile - 1) : analyze(n, m, Pp, Pi, Ap, Ai, tune, an, nwaves);
  if (rc) return rc;
  QPNumeric Q;
  load_qp(an, s, Pv, nullptr, Av, l, u, Q);
  if (s.scaling) scale_qp(an, s, Q);
  set_rho_vec(an, s, Q);
  std::vector<double> w;
  if ((rc = factor_qp(an, s, Q, w))) return rc;
  if (sol_direct) direct_kkt_solve(an, Q, rhs, sol_direct);
  if (sol_schedule && !replay_kkt_solve(an, Q, rhs, sol_schedule)) {
    g_last_error = "schedule streams are not race-free / deadlock-free"; return MI_OSQP_ERR_INVALID_DATA;
  }
  if (st) {
    memset(st, 0, sizeof(*st));
    st->n = n; st->m = m; st->N = an.N; st->batch = 1; st->tile = 1; st->n_tiles = 1;
    st->nnz_P_triu = an.Pp[n]; st->nnz_A = an.Ap[n]; st->nnz_KKT = an.nnzK(); st->nnz_L = an.nnzL();
    st->n_supernodes = (int64_t)an.sn_start.size() - 1; st->n_blocks = (int64_t)an.chunk_start.size() - 1;
    st->fwd_levels = an.fwd.n_phases; st->bwd_levels = an.bwd.n_phases;
    st->fwd_slots = (int64_t)an.fwd.phys_steps() * 64; st->bwd_slots = (int64_t)an.bwd.phys_steps() * 64; st->chk_slots = (int64_t)an.chk.phys_steps() * 64;
    st->dense_tail_rows = an.dt.k; st->dense_tail_slots = (int64_t)an.dt.n_steps * 64;
    st->nnz_L_before_tail = an.dt.k ? an.Lp[an.dt.s] : an.nnzL();
    st->threads_per_block = 64 * (tile > 1 ? 8 : nwaves);
    dense_tail_deal_stats(an.dt, *st);
  }
  return MI_OSQP_OK;
}

int mi_osqp_debug_host_block_factor(int64_t n, int64_t m, const int64_t *Pp, const int64_t *Pi, const double *Pv,
                                    const int64_t *Ap, const int64_t *Ai, const double *Av, const double *l,
                                    const double *u, const mi_osqp_settings *settings, double *dL, double *dD,
                                    int64_t *counts) {
  Settings s = to_settings(settings);
  if (validate_settings(s)) return MI_OSQP_ERR_INVALID_SETTINGS;
  Analysis an;
  int rc = analyze(n, m, Pp, Pi, Ap, Ai, tuning_from_env().analysis, an);
  if (rc) return rc;
  QPNumeric Q, R;
  load_qp(an, s, Pv, nullptr, Av, l, u, Q);
  if (s.scaling) scale_qp(an, s, Q);
  set_rho_vec(an, s, Q);
  std::vector<double> w;
  if ((rc = factor_qp(an, s, Q, w))) return rc;
  if ((rc = replay_block_factor(an, s, Q, R))) return rc;
  double mL = 0.0, sL = 1e-300, mD = 0.0;
  // with a dense tail the device factor holds L only for the columns before it (and S^-1 instead of the rest)
  const int ts = an.dt.k ? an.dt.s : an.N;
  for (int k = 0; k < an.Lp[ts]; k++) { mL = std::max(mL, std::fabs(Q.Lx[k] - R.Lx[k])); sL = std::max(sL, std::fabs(Q.Lx[k])); }
  for (size_t k = (size_t)an.nnzL(); k < Q.Lx.size(); k++) { mL = std::max(mL, std::fabs(Q.Lx[k] - R.Lx[k])); sL = std::max(sL, std::fabs(Q.Lx[k])); }
  for (int k = 0; k < ts; k++) mD = std::max(mD, std::fabs(Q.Dlinv[k] - R.Dlinv[k]) / std::fabs(Q.Dlinv[k]));
  if (an.dt.k) {
    double mM = 0.0, sM = 1e-300;
    for (size_t k = 0; k < Q.Minv.size(); k++) { mM = std::max(mM, std::fabs(Q.Minv[k] - R.Minv[k])); sM = std::max(sM, std::fabs(Q.Minv[k])); }
    mL = std::max(mL, mM / sM * sL);
  }
  if (dL) *dL = mL / sL;
  if (dD) *dD = mD;
  if (counts) {
    counts[0] = (int64_t)an.bf.n_blocks(); counts[1] = (int64_t)an.bf.tri.size() / 2;
    counts[2] = an.bf.storage; counts[3] = an.bf.n_levels;
  }
  return MI_OSQP_OK;
}

}  // extern "C"
