// npow_pool.cpp -- the work pool of libnanopow.so: every first-win search (npow_search,
// npow_search_batch, npow_submit) is a job; up to max_active jobs are searched at once,
// all of them by ONE kernel launch per device (npow_pool_kernel_ls2*), each on a disjoint
// per-device stride of its nonce space.
//
// Replaces the request queue and GPU loop of the reference work server
// (client/bin/windows/nano-work-server.exe, Rust source not vendored; behaviour from its
// strings): requests queue FIFO (@1681064 `--shuffle` is the server's choice of order),
// every GPU scans nonce chunks for the queued root, each GPU result is re-validated on the
// CPU ("GPU returned invalid work", @1669040; a GPU is dropped after 3 invalid results in a
// row, @1669144), and work_cancel ends the request with "Cancelled" (@1673856).
// The reference serves ONE root at a time; a DPoW burst (many work_generate requests in
// flight, client/work_handler.py:83-125 per client) is served here by keeping up to
// kMaxSlots roots live in every launch, so a root that is won mid-launch costs nothing:
// its workgroups move on to the other live roots (npow_kernel.hip, pool_body_ls2).
//
// This file: the pool, its jobs' state transitions, a GPU's Worker, and the device and pool lifecycle.
// npow_pool_jobs.cpp: the ticket calls behind the C ABI (submit, wait, cancel, promote, retarget, relax) and what they
// say of the three kinds of job; npow_pool_watch.cpp: the win watcher; npow_cpu.cpp: the CPU device;
// npow_pool_impl.h: what the pool's files share, the host's writes to a device's pinned mailbox among it (mb_kill,
// mb_boost, mb_floor, mb_yield).
//
// A job also leaves its launch early in both directions:
// a won or killed job finishes from the final nonce count the kernel publishes once no workgroup is
// left on its entry (Worker::early_finish; PoolMailbox::fin), and a new unbounded job joins the running
// launch as a dynamic entry (dyn_add; PoolMailbox::dyn) instead of ending it (yield_if_long, now
// the fallback).  DESIGN.md section 1.
//
// The worker's side of the collecting kinds of job (Job::kind; npow_pool_jobs.cpp has the callers' side): a sweep
// job's entries collect every hit of their ranges in the launch's hit records (PoolHits), which the worker reads as
// each launch retires (collect_hits, collect_sweep).  A best job's entries (kEntryBest) keep only the nonces
// that beat the best value their launch has seen: collect_best recomputes each record's value on the CPU and folds it
// into the job's best (npow_best.h), which the next entry carries as its watch.  A background job of either kind
// (Job::claimed()) is left out of a device's tables while a foreground job is live there (hold_out); its entries are
// claimed ones (kEntryClaim, beside kEntryBest for a best job): a launch covers a prefix of its span, told by its
// claim counter, and ends at the time budget or a yield; credit_entry, which both collectors call, credits the
// prefix and hands the rest back.  A shared job of either kind (Job::shared) has claimed entries too, but is a
// foreground job that no table leaves out: it weighs 1 in the start map of a table whose bounded entries are all
// claimed (build_table), and the kernel moves the workgroups its launch's searches no longer want to its entry.
//
// Threads: one persistent worker per device (started by npow_init) owns the device's
// stream, its slot table and up to two launches in flight (the second is queued only near
// the end of the first one's budget, or at once behind a launch with no live entry left);
// callers block in pool_wait.  The
// only cross-device datum is a job's outcome: the first device whose winner passes CPU
// re-validation decides the job, the others raise their slot's kill word (pinned host
// memory that the waves poll) and retire it.  No collective, no device-to-device traffic.
//
// Fault policy (per device, never per job): a device whose winners fail CPU re-validation 3
// times in a row (across jobs), or whose HIP calls fail, is marked dead: select_devices()
// skips it from then on, and every job it held hands the part of its nonce range the device
// had not finished to the job's surviving devices (re-striding; a bounded job's range stays
// covered exactly once more).  A job fails only when no device is left to search it.
// Test hooks (environment, read once, and only with NANOPOW_TEST_HOOKS=1 beside them -- a stray
// variable in a deployment must not drop GPUs; an active hook is reported on stderr):
// NANOPOW_FAULT_INVALID=d[,d...] makes the host read a corrupted value for every win of those
// logical devices; NANOPOW_FAULT_HIP=d:n makes device d's launches fail after its n-th;
// NANOPOW_FAULT_RETARGET_BLIND=1 makes pool_retarget skip the slots' floor records, so a running launch learns of
// a raise only through the host's refusal of its win (handle_win's stale path).
// NANOPOW_SHARED_NO_MOVES=1 turns the kernel's move to a claimed entry off (PoolTable::pad kTabNoMoves; A/B runs of
// shared range jobs).
// (npow_engine.cpp: NANOPOW_FAULT_INIT=d fails npow_init on d.)
#include <hip/hip_runtime.h>
#include <sys/prctl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "npow_pool_impl.h"

namespace npow {
namespace {

constexpr double kYieldMinUs = 1500.0;  // yield a running launch only if more budget than this is left
// ... and only if it holds fewer live unbounded jobs than this.  A new job then waits at most one
// launch budget (20 ms), small beside its time-to-work when it shares the GPU with 8+ others
// (>= 8 x ~19 ms at fffffff8), and a burst (64 live jobs, a win every ~20 ms) no longer ends
// every launch early: each early end costs the GPU the gap before the next launch starts.
constexpr int kYieldMaxLive = 8;
constexpr int kIdleSpinUs = 2000;       // an idle worker polls for new jobs this long before sleeping
constexpr double kPrelaunchUs = 2000.0;  // queue the next launch when the running one has this much budget left
constexpr double kDynMinUs = 3000.0;     // join a running launch only with this much budget left
constexpr double kFreshSpinUs = 400.0;   // poll without sleeping this long after a launch starts (quick wins)
constexpr int kInvalidStreakMax = 3;     // consecutive invalid results that drop a device (@1669144)
constexpr double kStopSpinUs = 2000.0;   // nap(): poll without sleeping this long after a slot's job stopped
// A slot whose job finished from its published final count is freed without reading its done counts back once the
// launches that held it have completed, except every kVerifyEvery-th, which still checks the count against the
// read-back (npow_device_stats.early_mismatches).  NANOPOW_READBACK=always reads every slot back (A/B runs).
constexpr uint64_t kVerifyEvery = 16;
constexpr int kLingerMaxCus = 32;  // lingering launches by default (npow_pool_impl.h g_linger_env)
bool lingers(const Device& d) {
  if (d.time_shared) return false;
  return g_linger_env >= 0 ? g_linger_env == 1 : (d.cu_first >= 0 && d.cus <= kLingerMaxCus);
}
}  // namespace
bool test_hooks_enabled() {
  static const bool on = [] {
    const char* e = getenv("NANOPOW_TEST_HOOKS");
    return e && strcmp(e, "1") == 0;
  }();
  return on;
}
const Faults& faults() {
  static const Faults f = [] {
    Faults x;
    if (!test_hooks_enabled()) {
      if (getenv("NANOPOW_FAULT_INVALID") || getenv("NANOPOW_FAULT_HIP") || getenv("NANOPOW_FAULT_RETARGET_BLIND"))
        fprintf(stderr, "nanopow: NANOPOW_FAULT_* ignored (test hooks need NANOPOW_TEST_HOOKS=1)\n");
      return x;
    }
    if (const char* e = getenv("NANOPOW_FAULT_INVALID")) {
      for (const char* p = e; *p;) {
        char* end = nullptr;
        const long d = strtol(p, &end, 10);
        if (end == p) break;
        if (d >= 0 && d < 64) x.invalid_mask |= 1ull << d;
        p = *end ? end + 1 : end;
      }
    }
    if (const char* e = getenv("NANOPOW_FAULT_HIP")) {
      char* end = nullptr;
      x.hip_dev = (int)strtol(e, &end, 10);
      if (end && *end == ':') x.hip_after = strtoull(end + 1, nullptr, 10);
    }
    if (const char* e = getenv("NANOPOW_FAULT_RETARGET_BLIND")) x.retarget_blind = strcmp(e, "1") == 0;
    if (const char* e = getenv("NANOPOW_SHARED_NO_MOVES")) x.no_moves = strcmp(e, "1") == 0;
    if (x.invalid_mask || x.hip_dev >= 0)
      fprintf(stderr, "nanopow: TEST HOOKS ACTIVE: corrupt wins of device mask %#llx, fail launches of device %d after %llu\n",
              (unsigned long long)x.invalid_mask, x.hip_dev, (unsigned long long)x.hip_after);
    if (x.retarget_blind) fprintf(stderr, "nanopow: TEST HOOKS ACTIVE: retargets write no floor record\n");
    if (x.no_moves) fprintf(stderr, "nanopow: TEST HOOKS ACTIVE: no workgroup moves to a claimed entry\n");
    return x;
  }();
  return f;
}

// -- jobs shared with the CPU workers (npow_pool.h) ---------------------------------------------
Pool g_pool;
std::atomic<uint64_t> g_gen{0};
std::atomic<bool> g_exiting{false};
std::atomic<double> g_exit_deadline_us{0.0};

// -- deferred notifications (PoolLock, npow_pool.h) ----------------------------------------------
namespace {
struct Deferred {
  int depth = 0;
  bool workers = false;
  std::vector<Job*> jobs;
};
thread_local Deferred t_defer;

void notify_waiters_now(Job& j) {
  { std::lock_guard<std::mutex> g(j.wmu); }  // a waiter between its check and its wait cannot miss the notify
  j.cv.notify_all();
}

void notify_workers_now() {
  g_pool.cv_work.notify_all();
  for (auto& dp : g_devs) wake_worker(*dp);
}
}  // namespace

void wake_worker(Device& d) {
  {
    std::lock_guard<std::mutex> g(d.wake_mu);
    ++d.wake_seq;
  }
  d.wake_cv.notify_one();
}

PoolLock::PoolLock() : lk_(g_pool.mu) { t_defer.depth++; }

PoolLock::~PoolLock() {
  lk_.unlock();
  if (--t_defer.depth > 0) return;
  // the states these wake-ups announce were all written under the lock: a thread woken now finds them
  std::vector<Job*> jobs;
  jobs.swap(t_defer.jobs);
  const bool workers = t_defer.workers;
  t_defer.workers = false;
  for (Job* j : jobs) notify_waiters_now(*j);
  if (workers) notify_workers_now();
}

// -- job state transitions (caller holds g_pool.mu) ------------------------------------------
static void notify_waiters(Job& j) {
  if (t_defer.depth > 0) {
    if (std::find(t_defer.jobs.begin(), t_defer.jobs.end(), &j) == t_defer.jobs.end()) t_defer.jobs.push_back(&j);
    return;
  }
  notify_waiters_now(j);
}

void notify_workers_locked() {
  if (t_defer.depth > 0) {
    t_defer.workers = true;
    return;
  }
  notify_workers_now();
}

void decide_locked(Job& j, int status, uint64_t nonce, uint64_t value) {
  if (j.status != kPending) return;
  j.status = status;
  j.nonce = nonce;
  j.value = value;
  j.decided.store(true, std::memory_order_release);  // the outcome above is read by waiters that acquire this
  notify_waiters(j);  // npow_wait_result returns at the decision
}

// The waiting queue's front while it may go live.  A foreground job: while fewer than max_active foreground jobs are
// live and a slot is free -- live background jobs do not count, so it never waits behind them.  A background job
// (they queue behind every foreground one, queue_rank): only while fewer than max_active jobs are live in all, and
// background jobs hold fewer than half of the slots.
constexpr size_t kMaxBackground = kMaxSlots / 2;
void admit_locked() {
  bool added = false;
  size_t bg = 0;
  for (const JobP& a : g_pool.active) bg += a->background ? 1u : 0u;
  while (!g_pool.waiting.empty() && g_pool.active.size() < (size_t)kMaxSlots) {
    const bool jbg = g_pool.waiting.front()->background;
    if (jbg ? (g_pool.active.size() >= g_pool.max_active || bg >= kMaxBackground)
            : (g_pool.active.size() - bg >= g_pool.max_active))
      break;
    JobP j = g_pool.waiting.front();
    bg += jbg ? 1u : 0u;
    g_pool.waiting.pop_front();
    j->admitted = true;
    g_pool.active.push_back(j);
    added = true;
  }
  if (added) {
    g_pool.version.fetch_add(1);
    notify_workers_locked();
  }
}

void finish_locked(const JobP& j) {
  if (j->finished) return;
  if (j->status == kPending) {
    if (j->cancel_seen()) j->status = NPOW_CANCELLED;
    else if (j->lost) j->status = j->lost_code;
    else j->status = NPOW_EXHAUSTED;
    j->decided = true;
  }
  j->t_finish = now_us();
  j->finished.store(true, std::memory_order_release);
  auto it = std::find(g_pool.active.begin(), g_pool.active.end(), j);
  if (it != g_pool.active.end()) g_pool.active.erase(it);
  auto wt = std::find(g_pool.waiting.begin(), g_pool.waiting.end(), j);
  if (wt != g_pool.waiting.end()) g_pool.waiting.erase(wt);
  admit_locked();
  notify_waiters(*j);
}

// Device k of job j is finished with it (retired, exhausted, or the device failed).
void device_done_locked(const JobP& j, size_t k, double t_seen) {
  JobDev& jd = j->dev[k];
  if (jd.done) return;
  jd.done = true;
  jd.on = false;
  if (jd.seen && jd.t_stop == 0) jd.t_stop = t_seen > 0 ? t_seen : now_us();
  if (--j->pending_devs == 0) finish_locked(j);
}

// Device k of job j is dead: hand the ranges it had not finished (its todo, including any a
// failed launch pushed back) to the job's surviving devices, split evenly (re-striding), then
// release it.  With no survivor the job has lost part of its nonce space and fails.
void abandon_locked(const JobP& j, size_t k, int code, const std::string& msg) {
  if (j->dev[k].done) return;
  std::deque<Range> rest;
  rest.swap(j->dev[k].todo);
  if (j->collects() && !j->decided) {
    // a sweep job's part is never hashed again on another device -- the hits the dead device had reported, or was
    // about to, would come twice: the job fails with the device's error, and its other devices stop
    j->err = msg;
    decide_locked(*j, code);
    g_pool.decisions.fetch_add(1, std::memory_order_release);
    notify_workers_locked();
  }
  if (!j->decided && !rest.empty()) {
    // the surviving GPUs take it; the CPU device (npow_cpu.cpp) only when no GPU of the job is left
    std::vector<size_t> surv, surv_cpu;
    for (size_t k2 = 0; k2 < j->devs.size(); ++k2) {
      const Device& d2 = *g_devs[(size_t)j->devs[k2]];
      if (k2 != k && !d2.dead) (d2.cpu_threads ? surv_cpu : surv).push_back(k2);
    }
    if (surv.empty()) surv.swap(surv_cpu);
    if (surv.empty()) {
      j->lost = true;
      j->lost_code = code;
      j->err = msg;
    } else {
      const uint64_t S = surv.size();
      for (const Range& r : rest) {
        uint64_t off = 0;
        for (uint64_t i = 0; i < S; ++i) {
          const uint64_t part = r.count / S + (i < r.count % S ? 1 : 0);
          if (part) j->dev[surv[i]].todo.push_back({r.base + off, part});
          off += part;
        }
      }
      for (size_t k2 : surv)
        if (j->dev[k2].done && !j->dev[k2].todo.empty()) {  // it had finished its own part: reopen
          j->dev[k2].done = false;
          ++j->pending_devs;
        }
      g_pool.version.fetch_add(1);
      notify_workers_locked();
    }
  }
  device_done_locked(j, k);
}

// Job j has just been decided by device k_win's result: raise the kill word of every other device
// that holds it now, instead of waiting for that device's worker to notice the decision at its next
// step (it naps up to g_poll_us between steps), and wake the napping workers.  A late store could not
// stop another job (mb_kill) -- and cannot happen anyway: a device releases a slot only under
// g_pool.mu, after device_done_locked or a re-arm cleared JobDev::on.
void stop_other_devices_locked(Job& j, size_t k_win) {
  if (j.devs.size() < 2) return;
  for_each_gpu_slot(j, [&](size_t k, Device& d, JobDev& jd) {
    if (k == k_win) return;
    mb_kill(d, jd.slot, jd.gen);
    std::lock_guard<std::mutex> sg(d.stats_mu);
    d.kills_relayed++;
  });
  g_pool.decisions.fetch_add(1, std::memory_order_release);
  notify_workers_locked();
}

void accept_win(Job& j, size_t k, uint64_t nonce, uint64_t value, double t_seen, uint64_t gpu_t) {
  decide_locked(j, NPOW_OK, nonce, value);
  j.t_decide = now_us();
  if (t_seen > 0) {
    j.t_win_seen = t_seen;
    if (j.t_win == 0) j.t_win = t_seen;
  }
  j.gpu_t_win = gpu_t;
  j.winner_k = (int)k;
  stop_other_devices_locked(j, k);
}

// Needs (under g_pool.mu): some active job wants this device.
bool wants_device_locked(int dev) {
  for (const JobP& j : g_pool.active) {
    const int k = index_in(*j, dev);
    if (k >= 0 && !j->dev[k].on && !j->dev[k].done) return true;
  }
  return false;
}

namespace {

// -- one device's worker ------------------------------------------------------------------------
enum class SlotState { kFree, kActive, kDraining };

// What a slot knows of the job it holds: adopt() resets all of it with one assignment.
struct Adoption {
  JobP job;
  size_t k = 0;            // the device's index within job->devs
  uint64_t gen = 0;
  bool win_seen = false;
  bool requeue = false;    // invalid GPU result: hand the job back to this device after retiring
  bool no_more = false;    // bounded range fully issued
  bool readback = false;   // done-shard read-back queued (ev_done[slot] marks it)
  bool no_readback = false;  // finished early and not sampled for verification: freed once inflight is empty
  bool fresh = false;      // adopted since the last launch was built
  bool held = false;       // a claimed job's slot left out of the tables: a foreground job wants the device
                           // (hold_out); it keeps its generation and its place in the range
  bool ending = false;     // a shared job's slot whose running launch was yielded (yield_if_long): nothing waits for
                           // that launch (live_slot), so the next table is queued behind it at once, and the slot is
                           // in it -- it is never held; cleared by its next entry (take_entry)
  uint64_t claimed = 0;    // a claimed job: the nonces its retired launches' claims covered in this generation
                           // (credit_entry), checked against the slot's done counts when it retires
  bool new_job = false;    // adopted for the first time on this device (not a re-adoption)
  bool fin_seen = false;   // the kernel published this generation's final count (PoolMailbox::fin) ...
  bool early = false;      // ... and the job was finished from it before retiring
  double stop_us = 0;      // the job was won or killed at this time: the worker polls without napping
                           // until the slot's final count is in (a quick return, and an exact stop time)
  bool stale = false;      // its final count had not come g_linger_us after stop_us (npow_device_stats.stale_drains)
  struct Issued { uint64_t seq, base, count; };
  std::vector<Issued> inflight;  // ranges handed to launches that have not completed (in order)
  uint64_t unread = 0;           // bounded job: nonces of its completed ranges whose done shards have not
                                 // been read back (a failed device's fail_all counts them from this)
};

struct Slot : Adoption {
  SlotState state = SlotState::kFree;
  // The device's counters of this slot index only grow: what they read at the slot's last crediting (credit_counts)
  uint64_t baseline = 0;    // done counter
  uint64_t late_base = 0;   // late counter (kLateWord)
  uint64_t stale_base = 0;  // stale-hit counter (kStaleWord)
};

struct Counts { uint64_t done, late, stale; };

struct PoolInflight {
  uint64_t seq;
  int ring;
  uint64_t dyn_base;    // PoolTable::dyn_base of the launch
  uint64_t yield_base;  // PoolTable::yield_base of the launch
  bool counted;         // PoolTable::counted: early finish and dynamic entries are on in it
  bool linger;          // PoolTable::linger: its workgroups wait for dynamic entries until its budget or a yield
  uint32_t wdown;       // its table's weights were halved this many times (pool_table_weights): its dynamic entries' too
  bool bounded;         // its table holds a bounded entry: no entry of the launch carries the background flag
  // Its collecting entries (sweep jobs): the slot and generation of each, and its region of the launch's hit records
  // (PoolHits; the set is ring & 1), `room` records from record region * room on.  Read when the launch retires.
  // A claimed entry (a background sweep or best job's, kEntryClaim) also has its span: the launch's claim counter of the slot
  // tells which prefix of it was covered (npow_claims.h).
  struct Collect {
    int slot;
    uint64_t gen;
    uint32_t region, room;
    bool claim;
    uint64_t base, count;
  };
  std::vector<Collect> collect;
  bool claimed() const {  // it holds a claimed entry: a foreground search does not join it, a yield ends it
    for (const Collect& c : collect)
      if (c.claim) return true;
    return false;
  }
};

// The most nonces a collecting entry of threshold `threshold` takes in one launch, so that its hits fit the `room`
// records of its region.  A launch's hits past its region are counted but not stored, and which ones are lost is up to
// the order its waves came in -- the job would keep its exact count but not its first hits.  The number of hits in
// `span` nonces is binomial with p = (2^64 - threshold) / 2^64: mean p * span and variance below the mean, so a span
// with mean + 8 sigma <= room (sigma <= sqrt(room)) overflows about once in 10^15 launches; with threshold 0 every
// nonce is a hit and the span is exact.  At the thresholds audits run with (p <= 2^-16) this is above every launch's
// span, and the bounded jobs' own span (PoolShape::own) is what a launch takes.
uint64_t collect_span(uint64_t threshold, uint32_t room) {
  const double p = threshold ? (double)(0 - threshold) / 18446744073709551616.0 : 1.0;
  const double fit = (double)room - 8.0 * std::sqrt((double)room) - 64.0;
  const double span = (fit > 64.0 ? fit : 64.0) / p;
  return span >= 9.0e18 ? ~0ull : (uint64_t)span;
}

class Worker {
 public:
  explicit Worker(Device& d) : d_(d) {}
  void run();

 private:
  Device& d_;
  Slot slots_[kMaxSlots];
  std::deque<PoolInflight> q_;
  std::vector<PoolInflight::Collect> collect_;  // build_table: the collecting entries of the table it built
  uint64_t seq_ = 0;  // launches issued by this worker
  uint64_t retired_seq_ = 0;  // the last launch retire_launches() has dropped (launches retire in order)
  uint64_t seen_version_ = ~0ull;
  int ring_ = 0;
  uint32_t mult_grid_ = 0, mult_ = 1;  // pool_claimed_mult of the device's grid (build_table)
  std::chrono::steady_clock::time_point front_start_{};  // host estimate of the running launch's start
  uint64_t ctl_ = 0;  // PoolMailbox::ctl (only this worker writes it): yields << 32 | dynamic entries
  uint64_t wake_seen_ = 0;  // Device::wake_seq as of this worker's last nap
  uint64_t early_count_ = 0;  // slots finished early so far (every kVerifyEvery-th is still read back)
  double idle_since_ = 0;     // launches in flight but no live slot since (end_linger after g_linger_us), 0 = busy
  double linger_t_ = 0;       // the last step that found a lingering launch idle (npow_device_stats.linger_ms), 0 = none
  int invalid_streak_ = 0;  // consecutive winners of this device that failed CPU re-validation
  int prev_stop_ring_ = -1;  // ring of the last retired launch (its stop event: the GPU idle before the next one),
                             // -1 when a sweep / values task used the device's events since
  uint64_t prev_g1_ = 0;     // NANOPOW_TRACE_LATENCY: the previous launch's end on the GPU clock
  struct StepProf {
    uint64_t n = 0, slow = 0;
    double total = 0, max = 0;
  };
  StepProf prof_[6];  // NANOPOW_TRACE_STEPS: adopt, check_slots, queue_readbacks, launch, retire, nap
  template <class F>
  auto timed(int part, F&& f) {
    if (!g_trace_steps) return f();
    const double t = now_us();
    auto r = f();
    const double dt = now_us() - t;
    StepProf& p = prof_[part];
    p.n++;
    p.total += dt;
    p.max = std::max(p.max, dt);
    if (dt > 50.0) p.slow++;
    return r;
  }
  void print_prof() const {
    static const char* names[6] = {"adopt", "check_slots", "read-back", "launch", "retire", "nap"};
    for (int i = 0; i < 6; ++i)
      fprintf(stderr, "nanopow-steps[%d] %-11s n %llu total_ms %.1f mean_us %.2f max_us %.1f over50us %llu\n", d_.id,
              names[i], (unsigned long long)prof_[i].n, prof_[i].total * 1e-3,
              prof_[i].n ? prof_[i].total / prof_[i].n : 0.0, prof_[i].max, (unsigned long long)prof_[i].slow);
  }
  std::unique_lock<std::mutex> dev_lock_{d_.mu, std::defer_lock};

  template <class F>
  void stat(F&& f) {  // the device's statistics (npow_device_stats_get reads them) change under their lock
    std::lock_guard<std::mutex> sg(d_.stats_mu);
    f();
  }
  void drop(int code, const std::string& msg) { d_.dead_code = code; d_.dead_msg = msg; d_.dead = true; }
  bool busy() const {
    if (!q_.empty()) return true;
    for (const Slot& s : slots_)
      if (s.state != SlotState::kFree) return true;
    return false;
  }
  bool live_slot(int except = -1) const {  // a slot (other than `except`) some launch in flight is hashing
    for (int s = 0; s < kMaxSlots; ++s)
      if (s != except && slots_[s].state == SlotState::kActive && !slots_[s].fresh && !slots_[s].held &&
          !slots_[s].ending)
        return true;
    return false;
  }
  // live_slot, of a foreground job (caller holds g_pool.mu: Job::background).  A shared range job is none here: the
  // background class shares its tables (hold_out), and a new background job ends its launch as it ends theirs
  // (a search that a yield handed back for re-adoption -- draining with `requeue`, undecided -- is still live: beside
  // a shared job, which is none, it would otherwise vanish between its yield and its next slot, and a background job
  // would slip into the table built in between)
  bool foreground_live(int except) const {
    for (int s = 0; s < kMaxSlots; ++s) {
      const Slot& sl = slots_[s];
      if (s == except || sl.state == SlotState::kFree || sl.job->background || sl.job->shared) continue;
      if (sl.state == SlotState::kActive ? !sl.fresh : (sl.requeue && !sl.job->decided.load())) return true;
    }
    return false;
  }
  double budget_left_us() const {  // of the running launch's time budget, by the host's estimate of its start
    return g_budget_us.load() -
           std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - front_start_).count();
  }
  // Slot s stops searching: with `kill`, its waves are told so; the watcher stops reading its job's cancel word.
  void stop_slot(int s, bool kill) {
    if (kill) mb_kill(d_, s, slots_[s].gen);
    slots_[s].state = SlotState::kDraining;
    watch_stop_cancel(d_, s);
  }
  void free_slot(int s) {
    watch_disarm(d_, s);
    slots_[s].job.reset();
    slots_[s].state = SlotState::kFree;
  }
  void adopt();
  void yield_if_long();
  void take_entry(Slot& sl, PoolEntry& pe, uint64_t want, uint64_t seq, double t);
  bool dyn_add(int s);
  void end_linger();
  void handle_win(int s);
  bool win_published(int s) const {
    return !slots_[s].win_seen && __atomic_load_n(&d_.pmb->win[s].gen, __ATOMIC_ACQUIRE) == slots_[s].gen;
  }
  Counts credit_counts(Slot& sl, uint64_t total, uint64_t late, uint64_t stale);
  static void credit_job_locked(const Slot& sl, const Counts& c) {
    sl.job->done += c.done;
    sl.job->dev[sl.k].late += c.late;
    sl.job->stale_hits += c.stale;
  }
  void early_finish(int s);
  // A stale slot's final count came after all (late): how late on the GPU's clock, after the job's deciding win at tw
  // (Job::gpu_t_win, read by the caller under g_pool.mu; npow_device_stats.stale_gpu_delay_us; one clock for CU
  // partitions of one GPU)
  void stale_fin_came(int s, uint64_t tw) {
    const uint64_t tf = __atomic_load_n(&d_.pmb->fin[s].t_fin, __ATOMIC_RELAXED);
    std::lock_guard<std::mutex> sg(d_.stats_mu);
    d_.stale_late++;
    if (tw && tf > tw) d_.stale_gpu_delay_us = std::max(d_.stale_gpu_delay_us, (double)(tf - tw) / 100.0);
  }
  void publish_busy() {
    int active = 0;
    for (const Slot& s : slots_) active += s.state == SlotState::kActive ? 1 : 0;
    d_.active_slots.store(active, std::memory_order_release);
    d_.worker_busy.store(busy(), std::memory_order_release);
  }
  // for pool_promote's count of promotions published into a running launch (npow_device_stats.promotions)
  void publish_counted() {
    int c = 0;
    for (const PoolInflight& f : q_) c += f.counted ? 1 : 0;
    d_.counted_inflight.store(c, std::memory_order_release);
  }
  void check_slots();
  void build_table(PoolTable& t, const int* idx, uint32_t n, bool* bounded);
  uint32_t hold_out(int* idx, uint32_t n);
  int launch(bool empty_linger = false);
  int queue_readbacks();
  int collect_hits(const PoolInflight& f);
  void collect_best(Slot& sl, const PoolInflight::Collect& c, const PoolInflight& f, uint64_t n, uint64_t stored);
  void credit_entry(Slot& sl, const PoolInflight::Collect& c, const PoolInflight& f);
  void collect_sweep(Slot& sl, const PoolInflight::Collect& c, const PoolInflight& f, uint64_t n, uint64_t stored);
  int retire_launches();
  int retire_slots();
  int retire() {
    DEVCHECK(d_, "pool retire");
    if (int rc = retire_launches()) return rc;
    return retire_slots();
  }
  void fail_all(const std::string& msg);
  uint64_t push_back_locked(Slot& sl, size_t from, bool skip_done = false);
  bool launch_completed(uint64_t seq) const;
  void account_clock(int ring, uint64_t seq, uint64_t* t0 = nullptr, uint64_t* t1 = nullptr);
  void trace_fin(int s) const;
  void trace_launch(const PoolInflight& f, uint64_t g0, uint64_t g1);
  void trace_nofin(int s, uint64_t seq) const;
  int step();
  void nap();
};

void Worker::adopt() {
  if (d_.dead) return;  // draining before it releases its jobs (run())
  const uint64_t v = g_pool.version.load();
  if (v == seen_version_) return;
  bool adopted = false;
  std::lock_guard<std::mutex> g(g_pool.mu);
  seen_version_ = g_pool.version.load();
  for (const JobP& j : std::vector<JobP>(g_pool.active)) {  // copy: device_done_locked may erase
    const int k = index_in(*j, d_.id);
    if (k < 0 || j->dev[k].on || j->dev[k].done) continue;
    JobDev& jd = j->dev[k];
    if (j->decided || jd.todo.empty()) {  // decided before this device got to it, or nothing left
      device_done_locked(j, k);
      continue;
    }
    int s = 0;
    while (s < kMaxSlots && slots_[s].state != SlotState::kFree) ++s;
    if (s == kMaxSlots) {  // cannot happen while max_active <= kMaxSlots; retry later
      seen_version_ = ~0ull;
      break;
    }
    Slot& sl = slots_[s];
    static_cast<Adoption&>(sl) = Adoption{};  // nothing of the slot's last job stays but the counters' baselines
    sl.state = SlotState::kActive;
    sl.job = j;
    sl.k = (size_t)k;
    sl.gen = ++g_gen;
    sl.fresh = true;
    jd.on = true;
    jd.slot = s;
    jd.gen = sl.gen;
    watch_arm(d_, s, sl.gen, j);
    if (j->t_adopt == 0) j->t_adopt = now_us();
    sl.new_job = !jd.seen;
    if (sl.new_job) adopted = true;  // a new job: worth ending a long launch for
    jd.seen = true;
  }
  // Unbounded jobs join the running launch as dynamic entries (no yield: the launch goes
  // on and workgroups move to them); a new job that cannot ends the long launch instead.
  bool waiting_new = false;
  const uint64_t ctl0 = ctl_;
  for (int s = 0; s < kMaxSlots; ++s) {
    Slot& sl = slots_[s];
    if (sl.state != SlotState::kActive || !sl.fresh) continue;
    // (a new background job that cannot join does not end a launch that hashes a foreground job: it waits for the
    // next table)
    if (!dyn_add(s) && sl.new_job && !(sl.job->background && foreground_live(s))) waiting_new = true;
  }
  // the entries published together (one release after all of them): workgroups of a lingering launch that see them
  // spread over all of them at once, where one at a time they would crowd onto the first and rebalance slowly
  if (ctl_ != ctl0) __atomic_store_n(&d_.pmb->ctl, ctl_, __ATOMIC_RELEASE);
  if (adopted && waiting_new) yield_if_long();
}

// Fill entry pe (of launch seq's table, or a dynamic entry of it) from the job of slot sl: its uniforms, threshold,
// generation and slot, and up to `want` nonces from the front of the device's queue of ranges, which then count as
// handed to that launch.  The caller sets pe.bounded and pe.wsh, and holds g_pool.mu (the job's queue and timestamps
// are shared with other workers).  t: now.
void Worker::take_entry(Slot& sl, PoolEntry& pe, uint64_t want, uint64_t seq, double t) {
  Job& j = *sl.job;
  JobDev& jd = j.dev[sl.k];
  memcpy(pe.u, j.u, sizeof(pe.u));
  pe.threshold = j.threshold;
  pe.reserve = j.armed ? j.reserve : pe.threshold;  // (no reserve: the waves' watch threshold is the entry's own)
  pe.gen = sl.gen;
  pe.slot = (uint32_t)(&sl - slots_);
  pe.bg = 0;
  if (jd.todo.empty()) jd.todo.push_back({j.start, 0});  // cannot happen (adopt / no_more); an empty entry
  Range& r = jd.todo.front();
  pe.base = r.base;
  pe.count = std::min(want, r.count);
  r.base += pe.count;
  r.count -= pe.count;
  if (r.count == 0) jd.todo.pop_front();
  sl.inflight.push_back({seq, pe.base, pe.count});
  if (j.t_launch == 0) j.t_launch = t;
  if (jd.t_launch == 0) jd.t_launch = t;
  if (jd.todo.empty()) sl.no_more = true;
  sl.fresh = false;
  sl.ending = false;
}

// Publish the job of fresh slot s as a dynamic entry of the running launch (npow_internal.h
// PoolDynEntry): exactly one launch in flight, enough of its budget left,
// not yielded, a free ring position, an unbounded job with a full region left, and either another live entry in it
// (workgroups to move) or a lingering launch (its workgroups wait for one).  Or (round 5) of the lingering launch
// queued behind an ending one whose ring is used up (step(): the replacement), at positions the ending one cannot
// read.  Its region is taken from the job's queue as launch() would, and counts as part of that launch.  Caller
// holds g_pool.mu (adopt()), and releases PoolMailbox::ctl after its calls.
bool Worker::dyn_add(int s) {
  Slot& sl = slots_[s];
  Job& j = *sl.job;
  if (q_.empty() || q_.size() > 2 || j.max_per_dev || g_budget_us.load() == 0) return false;
  const PoolShape sh = pool_shape(d_);
  const PoolInflight& f = q_.back();
  if (!f.counted) return false;  // a one-entry launch: the new job ends it (a yield) instead
  // a launch of claimed jobs (background sweep / best): its workgroups stay on their claimed entries until the spans
  // are used up, so a
  // foreground job that joined would wait for that; it ends the launch instead (a yield: within one chunk)
  if (f.claimed() && !j.background) return false;
  if ((uint32_t)((uint32_t)ctl_ - (uint32_t)f.dyn_base) >= (uint32_t)kDynEntries) return false;
  if ((ctl_ >> 32) != (f.yield_base >> 32)) return false;  // it is ending
  if (q_.size() == 2) {
    // the queued launch: a lingering one behind a launch that cannot see its ring positions (its own kDynEntries
    // were used up before this one was built: ring positions dyn_base .. dyn_base + kDynEntries - 1 of each, and
    // the ring holds both); it starts as soon as the other one's workgroups have left
    if (!f.linger || (uint32_t)(f.dyn_base - (uint32_t)q_.front().dyn_base) < (uint32_t)kDynEntries) return false;
  } else {
    // another live entry keeps the launch running (workgroups to move); else
    if (!live_slot(s) && !f.linger) return false;  // they are leaving: the next launch, right after, takes the job
    if (budget_left_us() < kDynMinUs) return false;  // the next launch, queued soon, takes it
  }
  const uint64_t full = sh.full(sh.launch_iters(g_iters.load()));
  const std::deque<Range>& todo = j.dev[sl.k].todo;
  if (todo.empty() || todo.front().count < full) return false;
  PoolEntry& pe = d_.pmb->dyn[(uint32_t)ctl_ % kDynRing].e;
  take_entry(sl, pe, full, f.seq, now_us());
  pe.bounded = 0;
  // the scaled balancing rule (ls2_poll) moves workgroups here up to its weighted share; on the table's scale
  pe.wsh = pool_wsh((j.weight >> f.wdown) ? (j.weight >> f.wdown) : 1u);
  // a background job (weight 1): parked until the launch's foreground entries end -- but in a launch whose table
  // holds a bounded entry it runs as a foreground job of weight 1, as the table's own do (build_table)
  pe.bg = j.background && !f.bounded ? 1u : 0u;
  if (pe.bg) pe.wsh = kWshOne | kWshBg;
  ctl_ = (ctl_ & ~0xffffffffull) | (uint32_t)(ctl_ + 1);  // the low half wraps on its own (released by adopt())
  stat([&] { d_.dyn++; });
  NPOW_DBGT("nanopow[%d]: dynamic entry %u: slot %d g%llu in launch %llu\n", d_.id, (uint32_t)ctl_ - 1u,
           s, (unsigned long long)sl.gen, (unsigned long long)f.seq);
  return true;
}

// New jobs wait for the next launch's table.  Launches run for a long time budget (their start costs ~0.1-0.2 ms of
// cold instruction/scalar caches, so long launches are faster), so when the running launch still has a while to go, end
// its unbounded entries now: a yield (polling waves mark those entries dead), and hand their jobs back for re-adoption
// with new generations next to the new ones.
void Worker::yield_if_long() {
  if (q_.empty() || g_budget_us.load() == 0) return;
  const double left_us = budget_left_us();
  NPOW_DBG("nanopow[%d]: yield? inflight %zu left_us %.0f\n", d_.id, q_.size(), left_us);
  if (q_.size() < 2 && left_us < kYieldMinUs) return;
  int live = 0;
  for (const Slot& sl : slots_)
    if (sl.state == SlotState::kActive && !sl.fresh && !sl.job->max_per_dev) ++live;
  // (a launch of claimed jobs is ended whatever it holds: nothing foreground is in it -- hold_out -- and the
  // job that waits cannot join it)
  bool claimed = false;
  for (const PoolInflight& f : q_) claimed = claimed || f.claimed();
  if (live >= kYieldMaxLive && !claimed) return;
  bool any = false;
  for (int s = 0; s < kMaxSlots; ++s) {
    Slot& sl = slots_[s];
    // a claimed job (background sweep / best) in the running launch: the yield ends its claims; the slot stays as it
    // is, and what the
    // launch did not reach goes back to the job when the launch retires (collect_hits)
    // (held from now on, as hold_out holds it: the next table is queued behind the ending launch at once -- live_slot)
    // (a shared job is not held: its slot goes into that next table, beside the job that waits -- `ending`)
    if (sl.state == SlotState::kActive && !sl.inflight.empty() && sl.job->claimed()) {
      any = true;
      if (sl.job->shared) {
        sl.ending = true;
      } else {
        if (!sl.held) sl.job->dev[sl.k].held_since = now_us();
        sl.held = true;
      }
    }
    if (sl.state != SlotState::kActive || sl.fresh || sl.job->max_per_dev) continue;
    sl.requeue = true;
    stop_slot(s, false);
    any = true;
  }
  NPOW_DBG("nanopow[%d]: yield %s\n", d_.id, any ? "raised" : "(no slot to hand back)");
  if (any) {
    mb_yield(d_, ctl_);
    std::lock_guard<std::mutex> sg(d_.stats_mu);
    d_.yields++;
  }
}

// A win published for slot s (this generation): CPU re-validation decides the job.
void Worker::handle_win(int s) {
  const double t_seen = now_us();
  Slot& sl = slots_[s];
  Job& j = *sl.job;
  sl.win_seen = true;
  uint64_t n, v;
  read_win(d_, s, &n, &v);
  const uint64_t cpu_v = host_work_value(j.pre.m, n);
  PoolLock g;  // (the slot holds the job)
  if (j.t_win == 0) j.t_win = t_seen;
  const uint64_t threshold = j.threshold.load(std::memory_order_relaxed);  // (under the lock: pool_retarget)
  if (cpu_v == v && v >= threshold) {
    invalid_streak_ = 0;
    if (j.status == kPending) accept_win(j, sl.k, n, v, t_seen, __atomic_load_n(&d_.pmb->win[s].t, __ATOMIC_RELAXED));
  } else {
    // "GPU returned invalid work": the launches that held this generation stopped at the win,
    // so a bounded job gets back every range from the one holding the winner on; the job is
    // re-armed on this device after the slot retires.  The third in a row drops the device.
    // A stale win -- the value is the CPU's, but below a threshold raised while the search ran (npow_retarget; the
    // wave read the slot's floor record before the host's store landed, or never could: a dropped record) -- is
    // correct work at the wrong difficulty, not a fault: it takes the same way back without touching the
    // device's invalid count or its streak.  (Only a job whose threshold was raised: a correct value below a
    // threshold that never moved is a kernel's fault like any other.)
    const bool stale = cpu_v == v && j.retargets > 0;
    if (stale) {
      j.stale_wins++;
      NPOW_DBGT("nanopow[%d]: slot %d g%llu: win %016llx below the raised threshold, re-armed\n", d_.id, s,
                (unsigned long long)sl.gen, (unsigned long long)v);
    } else {
      stat([&] { d_.invalid++; });
      fprintf(stderr, "nanopow: GPU %d returned invalid work %016llx (value %016llx, cpu %016llx)\n", d_.id,
              (unsigned long long)n, (unsigned long long)v, (unsigned long long)cpu_v);
    }
    if (j.max_per_dev) {
      size_t from = 0;
      for (size_t i = 0; i < sl.inflight.size(); ++i)
        if (n - sl.inflight[i].base < sl.inflight[i].count) {
          from = i;
          break;
        }
      push_back_locked(sl, from);
    }
    sl.requeue = true;
    if (!stale && ++invalid_streak_ >= kInvalidStreakMax && !d_.dead) {
      drop(NPOW_ERR_INVALID_WORK, "GPU " + std::to_string(d_.id) + " returned invalid work " +
                                      std::to_string(kInvalidStreakMax) + " consecutive times");
      fprintf(stderr, "nanopow: %s, dropping it\n", d_.dead_msg.c_str());
    }
  }
  stop_slot(s, false);  // the winning wave already marked the slot dead on the device
  sl.stop_us = now_us();
}

// Ranges sl.inflight[from..] did not complete (their launches stopped on this generation or
// failed): hand them back to the front of the job's queue for this device, in order.  With
// skip_done, a range whose launch has already completed on the GPU (retire_launches() has not seen it yet)
// stays: it was hashed in full, and handing it back would hash it again and over-count the job's
// nonces_done (a dropped device's check_slots / fail_all).  Returns the nonces of the ranges kept.
uint64_t Worker::push_back_locked(Slot& sl, size_t from, bool skip_done) {
  Job& j = *sl.job;
  std::vector<Slot::Issued> keep(sl.inflight.begin(), sl.inflight.begin() + (ptrdiff_t)from);
  uint64_t kept = 0;
  for (size_t i = sl.inflight.size(); i > from; --i) {
    const Slot::Issued& r = sl.inflight[i - 1];
    if (skip_done && launch_completed(r.seq)) {
      keep.insert(keep.begin() + (ptrdiff_t)from, r);
      kept += r.count;
      continue;
    }
    j.dev[sl.k].todo.push_front({r.base, r.count});
  }
  sl.inflight.swap(keep);
  return kept;
}

// The launch with sequence number seq has completed on the GPU: retire_launches() has dropped it, or its stop event has
// fired.  A launch whose issue failed (its ranges were assigned, then the HIP call failed: never in q_) has not.
bool Worker::launch_completed(uint64_t seq) const {
  if (seq <= retired_seq_) return true;
  (void)check_device(d_, "launch_completed");
  for (const PoolInflight& f : q_)
    if (f.seq == seq) return hipEventQuery(d_.ev_stop[f.ring]) == hipSuccess;
  return false;
}

// The launch's in-kernel clock records (PoolClk, one per XCD) into the device statistics.
void Worker::account_clock(int ring, uint64_t seq, uint64_t* t0, uint64_t* t1) {
  double cyc = 0, ref = 0;
  for (int x = 0; x < kClkWaves; ++x) {
    const PoolClk& c = d_.pmb->clk[ring][x];
    if (__atomic_load_n(&c.seq, __ATOMIC_ACQUIRE) != (uint32_t)seq) continue;
    if (t0) {  // the launch's span on the GPU's realtime clock: the earliest start, the latest end of the records
      const uint64_t a = __atomic_load_n(&c.t0, __ATOMIC_RELAXED), b = __atomic_load_n(&c.t1, __ATOMIC_RELAXED);
      if (*t0 == 0 || a < *t0) *t0 = a;
      if (b > *t1) *t1 = b;
    }
    const double cy = (double)__atomic_load_n(&c.cycles, __ATOMIC_RELAXED);
    const double rf = (double)__atomic_load_n(&c.ref, __ATOMIC_RELAXED);
    // a record from a wave that ran for a few ticks only (a launch that found its job already over) is
    // too coarse to price, and a clock outside 0.3-4 GHz is not a clock: skip both
    if (rf < 1000.0 || cy < 3.0 * rf || cy > 40.0 * rf) continue;
    cyc += cy;
    ref += rf;
  }
  std::lock_guard<std::mutex> sg(d_.stats_mu);
  d_.clk_ticks += cyc;
  d_.clk_ref_ticks += ref;
}

// The device's counters of sl's slot index read total / late / stale now: credit what they gained since the slot's
// last crediting to the device's statistics, move the baselines up, and return the gains for the job
// (credit_job_locked, under g_pool.mu).
Counts Worker::credit_counts(Slot& sl, uint64_t total, uint64_t late, uint64_t stale) {
  const Counts c{total - sl.baseline, late - sl.late_base, stale - sl.stale_base};
  sl.baseline = total;
  sl.late_base = late;
  sl.stale_base = stale;
  std::lock_guard<std::mutex> sg(d_.stats_mu);
  d_.nonces += c.done;
  d_.late += c.late;
  return c;
}

// NANOPOW_TRACE_LATENCY: the GPU timeline of slot s's final count (one GPU's clock: CU partitions), from the job's
// deciding win.  Caller holds g_pool.mu.
void Worker::trace_fin(int s) const {
  const Slot& sl = slots_[s];
  const Job& j = *sl.job;
  const double tw = (double)j.gpu_t_win, tr = (double)__atomic_load_n(&d_.pmb->fin[s].t_relay, __ATOMIC_RELAXED);
  fprintf(stderr, "[%.3f] nanopow-fin dev %d ticket %llu: relay %+.1f fin %+.1f seen %+.1f us (host) from the win%s\n",
          now_us() * 1e-3, d_.id, (unsigned long long)j.ticket, (tr - tw) / 100.0,
          ((double)__atomic_load_n(&d_.pmb->fin[s].t_fin, __ATOMIC_RELAXED) - tw) / 100.0,
          j.t_win_seen > 0 ? now_us() - j.t_win_seen : -1.0, (int)sl.k == j.winner_k ? " (winner)" : "");
#ifdef NPOW_DIAG_TIMES
    // absolute GPU times (100 MHz) of this entry's last start and its win, host times (us) of its launch / dynamic
    // entry and of its win seen: a serial client's gap between one search's win and the next one's hashing
  fprintf(stderr, "nanopow-join dev %d ticket %llu: gpu_join %llu gpu_win %llu host_launch %.1f host_win_seen %.1f\n",
          d_.id, (unsigned long long)j.ticket,
          (unsigned long long)__atomic_load_n(&d_.pmb->fin[s].t_join, __ATOMIC_RELAXED),
          (unsigned long long)j.gpu_t_win, j.dev[sl.k].t_launch, j.t_win_seen);
  // every workgroup's last entry start (a serial client: this search's) -- its spread
  std::vector<uint64_t> tj;
  const int G = ls_grid(d_) < 1024 ? ls_grid(d_) : 1024;
  for (int g = 0; g < G; ++g) tj.push_back(__atomic_load_n(&d_.pmb->diag_join[g], __ATOMIC_RELAXED));
  std::sort(tj.begin(), tj.end());
  fprintf(stderr, "nanopow-joins dev %d ticket %llu: min %llu p10 %llu p50 %llu p90 %llu max %llu\n", d_.id,
          (unsigned long long)j.ticket, (unsigned long long)tj[0], (unsigned long long)tj[G / 10],
          (unsigned long long)tj[G / 2], (unsigned long long)tj[G * 9 / 10], (unsigned long long)tj[G - 1]);
#endif
}

// The kernel published slot s's final nonce count (npow_kernel.hip "Early
// finish"): no workgroup is on the entry and none can join it, so a decided job is finished now
// instead of after the launch -- which its other entries may keep running for the rest of its
// budget.  A yielded entry (the job is re-adopted) or an invalid win (re-armed) waits for retire_slots().
void Worker::early_finish(int s) {
  const double t_obs = now_us();  // the device's stop as this worker saw it (not when it got the pool lock)
  Slot& sl = slots_[s];
  sl.fin_seen = true;
  if (win_published(s)) handle_win(s);  // the winner released its record before closing the entry
  const uint64_t total = __atomic_load_n(&d_.pmb->fin[s].total, __ATOMIC_RELAXED);
  const uint64_t late = __atomic_load_n(&d_.pmb->fin[s].late, __ATOMIC_RELAXED);
  const uint64_t stale_hits = __atomic_load_n(&d_.pmb->fin[s].stale, __ATOMIC_RELAXED);
  PoolLock g;  // (the slot holds the job)
  Job& j = *sl.job;
  if (g_trace_lat && j.gpu_t_win) trace_fin(s);
  if (__atomic_load_n(&d_.pmb->fin[s].linger_gen, __ATOMIC_RELAXED) == sl.gen)  // relayed by a lingering workgroup
    stat([&] { d_.linger_relays++; });
  if (sl.stale) stale_fin_came(s, j.gpu_t_win);
  if (d_.dead || sl.requeue || !j.decided.load()) return;
  if (j.collects()) return;  // a cancelled sweep job: the hits of the launches that held it are read as they retire
                        // (collect_hits), so the slot goes the read-back's way (retire_slots)
  sl.early = true;
  credit_job_locked(sl, credit_counts(sl, total, late, stale_hits));  // retire_slots() then reads back the same total
  if (g_trace_lat && j.t_kend == 0) j.t_kend = now_us();
  stat([&] { d_.early++; });
  device_done_locked(sl.job, sl.k, t_obs);
}

void Worker::check_slots() {
  for (int s = 0; s < kMaxSlots; ++s) {
    Slot& sl = slots_[s];
    if (sl.state == SlotState::kFree) continue;
    if (win_published(s)) {
      handle_win(s);
      continue;
    }
    if (sl.state != SlotState::kActive) continue;
    Job& j = *sl.job;
    if (d_.dead) {  // dropped device: stop every job's waves; retire_slots() re-strides them
      if (j.max_per_dev) {  // the killed launches leave their ranges unfinished: hand them back
        std::lock_guard<std::mutex> g(g_pool.mu);
        push_back_locked(sl, 0, true);
      }
      stop_slot(s, true);
    } else if (j.decided.load(std::memory_order_relaxed) || j.cancel_seen()) {
      {
        PoolLock g;  // (the slot holds the job)
        if (!j.decided.load()) {
          j.cancel_req = true;
          decide_locked(j, NPOW_CANCELLED);
        }
        // No launch holds the job on this device (adopted, waiting for the next launch's table): it hashes
        // nothing more of it, from now.  Otherwise the stop time (JobDev::t_stop) is taken when this worker sees
        // it stop hashing: its final count published, or the last launch that held it completed (retire_launches()).
        // A launch queued behind another and started after the kill still hashes the job until one of its
        // waves polls the kill word (within an iteration), so "not started at the decision" is no proof of zero.
        if (sl.inflight.empty() && j.dev[sl.k].t_stop == 0) j.dev[sl.k].t_stop = now_us();
      }
      stop_slot(s, true);  // in-flight waves stop
      sl.stop_us = now_us();
    } else if (sl.no_more && !(j.claimed() && !sl.inflight.empty())) {
      // (a claimed job's launches may hand part of their spans back: its slot stays until they have retired)
      if (sl.held) {  // (held at a yield, and the launches covered all that was left)
        std::lock_guard<std::mutex> g(g_pool.mu);
        JobDev& jd = j.dev[sl.k];
        jd.held_us += now_us() - jd.held_since;
        jd.held_since = 0;
        sl.held = false;
      }
      stop_slot(s, false);
    }
  }
  publish_busy();  // before a job can finish early: its waiter may read the stats at once
  for (int s = 0; s < kMaxSlots; ++s) {
    const Slot& sl = slots_[s];
    if (sl.state == SlotState::kDraining && !sl.fin_seen &&
        __atomic_load_n(&d_.pmb->fin[s].gen, __ATOMIC_ACQUIRE) == sl.gen)
      early_finish(s);
  }
}

// No live entry in the launches in flight, and something waits for the device (a job that could not join them, a
// sweep / values task, shutdown, a dropped device): a lingering launch would hold the device until its budget ends
// (up to 20 ms), so end it now -- a yield, which its lingering workgroups read
// within a look (ls2_linger) and which ends nothing else, no entry being live.  Raised before the next table is built
// (launch() takes yield_base after it), so that launch is not ended too.
void Worker::end_linger() {
  bool lingering = false;
  for (const PoolInflight& f : q_) lingering = lingering || (f.linger && (f.yield_base >> 32) == (ctl_ >> 32));
  if (!lingering) return;
  mb_yield(d_, ctl_);
  NPOW_DBGT("nanopow[%d]: lingering launch ended (ctl %llx)\n", d_.id, (unsigned long long)ctl_);
  std::lock_guard<std::mutex> sg(d_.stats_mu);
  d_.linger_ends++;
}

// The table of launch ++seq_ over the n slots idx[]: their entries (take_entry), the start map, the lingering mode.
void Worker::build_table(PoolTable& t, const int* idx, uint32_t n, bool* bounded) {
  const PoolShape sh = pool_shape(d_);
  const uint32_t iters = sh.launch_iters(g_iters.load());
  uint32_t wdown = 0;
  uint32_t weights[kMaxSlots], wshs[kMaxSlots];
  uint8_t bgs[kMaxSlots], kinds[kMaxSlots];
  t.n = n;
  t.poll_mask = poll_mask();
  t.iters = iters;
  t.budget = g_budget_us.load() * 100u;  // s_memrealtime runs at 100 MHz
  t.yield_base = ctl_;
  t.dyn_base = (uint32_t)ctl_;
  // One entry: the launch ends with it, and counting workgroups on it only delays that end (the
  // final count would reach the host ~60 us after the launch's own end; measured with
  // NANOPOW_TRACE_LATENCY).  Two or more: a won entry's job need not wait for the others.  A lingering launch is
  // counted from its first entry (set below, once the entries are known to be unbounded).
  t.counted = n >= 2 ? 1u : 0u;
  t.linger = 0;
  t.kill_base = (uint32_t)__atomic_load_n(&d_.pmb->kills, __ATOMIC_ACQUIRE);
  ++seq_;
  t.ring = (uint32_t)ring_;
  t.seq = (uint32_t)seq_;
  {
    std::lock_guard<std::mutex> g(g_pool.mu);  // issued[] is shared with other workers' reads
    // the promotion counter with the jobs' weights, both under the pool lock (pool_promote writes them under it): a
    // promotion is either in the weights read below or bumps the counter past this base, which the kernel then sees
    t.promo_base = (uint32_t)(__atomic_load_n(&d_.pmb->kills, __ATOMIC_ACQUIRE) >> 32);
    const double t_issue = now_us();
    const uint64_t full = sh.full(iters);
    // the table's collecting entries (sweep jobs) share the launch's hit records in 2^cshift equal regions
    uint32_t ncollect = 0, cshift = 0;
    for (uint32_t e = 0; e < n; ++e) ncollect += slots_[idx[e]].job->collects() ? 1u : 0u;
    while ((1u << cshift) < ncollect) ++cshift;
    collect_.clear();
    // A shared range job beside other entries: every claimed entry of the table takes a full launch region, as an
    // unbounded entry does, capped as below -- its workgroups are its share of the start map and then every workgroup
    // the launch's searches no longer want (ls2_move_claimed), so they must not run out of chunks before the launch's
    // time budget; what the launch does not claim goes back to the job (credit_entry).  Unless the table holds a dense
    // entry: it is dealt g % n then, and the entry's own share (PoolShape::own) is what its workgroups can cover.
    bool shared = false, dense_any = false;
    for (uint32_t e = 0; e < n; ++e) {
      const Slot& sl = slots_[idx[e]];
      const Job& j = *sl.job;
      const std::deque<Range>& todo = j.dev[sl.k].todo;
      shared = shared || (j.collects() && j.shared);
      dense_any = dense_any || (j.collects() ? !j.claimed() : (j.max_per_dev || todo.empty() || todo.front().count < full));
    }
    const bool wide = shared && !dense_any && n >= 2;
    for (uint32_t e = 0; e < n; ++e) {
      Slot& sl = slots_[idx[e]];
      const Job& j = *sl.job;
      const std::deque<Range>& todo = j.dev[sl.k].todo;
      if (j.collects()) {
        // the span a bounded job takes, unless the threshold is so low that its hits would not fit the region
        // (a best job's records are rare whatever its floor: the bounded span, and its best so far as the watch)
        const uint32_t room = kSweepHits >> cshift, region = (uint32_t)collect_.size();
        const uint64_t span = j.is_best() ? ~0ull : collect_span(j.threshold, room);
        take_entry(sl, t.e[e], std::min(wide && j.claimed() ? full : sh.own(e, n, iters), span), seq_, t_issue);
        if (j.is_best()) t.e[e].threshold = t.e[e].reserve = best_watch(j.best.of, j.threshold);
        t.e[e].bounded = pool_collect_flags(region, cshift) | (j.claimed() ? kEntryClaim : 0u) |
                         (j.is_best() ? kEntryBest : 0u);
        t.e[e].wsh = pool_wsh(j.weight);
        weights[e] = j.weight;
        bgs[e] = 0;
        kinds[e] = j.claimed() ? kTableClaimed : kTableDense;
        *bounded = true;
        collect_.push_back({idx[e], sl.gen, region, room, j.claimed(), t.e[e].base, t.e[e].count});
        continue;
      }
      // the next part of the device's queue of ranges: a bounded job's own waves cover it
      // densely; an unbounded job claims a full launch region (W * iters * 64, holes allowed)
      // unless less than that is left, which then becomes a dense bounded entry too
      const bool dense = j.max_per_dev || todo.empty() || todo.front().count < full;
      take_entry(sl, t.e[e], dense ? sh.own(e, n, iters) : full, seq_, t_issue);
      t.e[e].bounded = dense ? 1 : 0;
      t.e[e].wsh = pool_wsh(j.weight);
      weights[e] = j.weight;
      bgs[e] = j.background ? 1 : 0;
      kinds[e] = dense ? kTableDense : kTableUnbounded;
      *bounded = *bounded || dense;
    }
  }
  // The start map (PoolTable::wsum): workgroup g starts on the entry whose run of the cumulative weights holds
  // pool_start_pos(g, wsum), so every launch begins at its jobs' weighted shares (the kernel balances only toward
  // dynamic entries: a table dealt g % n would never reach them).  Equal weights, or a bounded entry (dense over
  // g % n == e): g % n.  Only differing weights need the map, and a workgroup must start on every entry, or that
  // entry would stay without one: pool_table_weights (npow_weights.h) halves a crowded table's weights until so.
  t.wsum = 0;
  uint32_t claimed_map = 0;
  if (!*bounded) {
    // (background jobs, pool_table_weights_bg: weight 0 in a map beside foreground ones, g % n among themselves.  A
    // table with a bounded entry carries no background flag -- take_entry cleared it: its background jobs run as
    // foreground jobs of weight 1 for this launch, since g % n starts workgroups on them)
    t.wsum = pool_table_weights_bg(weights, bgs, n, (uint32_t)sh.grid, wshs, &wdown);
    for (uint32_t e = 0; e < n; ++e) {
      t.e[e].wsh = wshs[e] | (bgs[e] ? kWshBg : 0u);
      t.e[e].bg = bgs[e];
    }
  } else {
    // (a table whose bounded entries are all claimed -- shared range jobs, the background class -- has a map too,
    // over its jobs' weights: a claimed entry takes its chunks from a counter and nothing from g % n.  Equal weights,
    // as in every table of the background class alone, still give g % n, and a table with a dense entry always does:
    // pool_table_weights_claimed, npow_weights.h.  The background flags stay cleared as above.)
    // Dealt by the claimed map, which is exact to a workgroup (PoolTable::pad carries its modulus and multiplier, wsum
    // stays 0: only the bounded kernels deal it).
    if (mult_grid_ != (uint32_t)sh.grid) {  // (a search over grid / 4 candidates: once per grid)
      mult_grid_ = (uint32_t)sh.grid;
      mult_ = pool_claimed_mult(mult_grid_);
    }
    const uint32_t mult = mult_;
    const uint32_t csum = pool_table_weights_claimed(weights, kinds, n, (uint32_t)sh.grid, mult, wshs, &wdown);
    for (uint32_t e = 0; e < n; ++e) t.e[e].wsh = wshs[e];
    if (csum) claimed_map = pool_claimed_pad(csum, mult);
  }
  t.wdown = wdown;  // (a promoted weight is published raw: the kernel halves it as the table's were, pool_promoted_wsh)
  t.pad = (faults().no_moves ? kTabNoMoves : 0u) | claimed_map;
  if (lingers(d_) && !*bounded && g_budget_us.load() > 0) {
    // each lingering workgroup reads the pinned ctl word once in P looks (phase g): ~2 reads per look grid-wide
    uint32_t P = 1;
    while (P * 2 < (uint32_t)sh.grid) P <<= 1;
    if (g_linger_p > 0) P = g_linger_p;
    t.linger = P;
    t.counted = 1u;
  }
}

// Claimed jobs (background sweep jobs, background best jobs) among the slots idx[] of the next table: while a
// foreground job is live on this device -- in a launch in flight, or among idx[] itself, waiting for this table --
// their slots are left out of it (and of live_slot(): nothing waits for them).  They keep their generation and their
// queue of ranges; the time they sit out is the job's held_us (npow_ticket_sweep, npow_ticket_best_hold).  Returns
// the new n.
uint32_t Worker::hold_out(int* idx, uint32_t n) {
  std::lock_guard<std::mutex> g(g_pool.mu);  // Job::background of the searches (pool_promote), JobDev
  bool fg = foreground_live(-1);  // (a shared range job is no foreground job here: it never starves the class)
  for (uint32_t e = 0; e < n && !fg; ++e) fg = !slots_[idx[e]].job->background && !slots_[idx[e]].job->shared;
  const double t = now_us();
  uint32_t m = 0;
  for (uint32_t e = 0; e < n; ++e) {
    Slot& sl = slots_[idx[e]];
    if (!sl.job->held_class()) {  // (a shared job's slot is never held)
      idx[m++] = idx[e];
      continue;
    }
    JobDev& jd = sl.job->dev[sl.k];
    if (fg) {
      if (!sl.held) jd.held_since = t;
      sl.held = true;
      continue;
    }
    if (sl.held) {
      jd.held_us += t - jd.held_since;
      jd.held_since = 0;
      sl.held = false;
    }
    idx[m++] = idx[e];
  }
  return m;
}

int Worker::launch(bool empty_linger) {
  if (q_.size() >= 2 || d_.dead) return NPOW_OK;
  // The second launch in flight only has to be queued before the running one ends (its budget
  // is known): queued early, it would sit behind a launch that a win ends, and the job could
  // only be retired after it too had started and drained (~20 us of every search's latency).
  // ... unless no live entry is left in it (its jobs won or were killed: it ends within a hash, and a
  // job finished early returns before that) -- then the next launch queues behind it at once.
  if (q_.size() == 1 && g_budget_us.load() > 0 && budget_left_us() > kPrelaunchUs && live_slot()) return NPOW_OK;
  uint32_t n = 0;
  int idx[kMaxSlots];
  bool claimed = false;  // (Job::sweep and a sweep job's class never change: read without the pool lock)
  for (int s = 0; s < kMaxSlots; ++s)
    if (slots_[s].state == SlotState::kActive && !slots_[s].no_more) {
      idx[n++] = s;
      claimed = claimed || slots_[s].job->held_class();
    }
  if (claimed) n = hold_out(idx, n);
  if (n == 0 && !empty_linger) return NPOW_OK;
  if (!live_slot()) end_linger();  // (step() has raised it already when a job waits; a bounded range's next part)
  PoolTable& t = *d_.h_tab[ring_];
  bool bounded = false;
  build_table(t, idx, n, &bounded);
  if (n == 0 && !t.linger) return NPOW_OK;
  const PoolShape sh = pool_shape(d_);
  const int r = ring_;
  ring_ = (ring_ + 1) % kEventRing;
  const size_t bytes = pool_table_bytes(n);
  DEVCHECK(d_, "pool launch");
  // Up to kArgEntries entries the table rides in the kernel arguments (no copy before the launch;
  // uploading it instead cost 2.5 %, profiles/r02_ab_table_upload.jsonl); a larger one goes up in
  // stream order right before its launch.  (Uploading it on a second stream beside the running
  // launch, joined by an event, cost 1.5-2 % of kernel throughput: the copy is a blit kernel that
  // competes with the running launch.)
  if (faults().hip_dev == d_.id && seq_ > faults().hip_after)  // NANOPOW_FAULT_HIP (tests)
    return fail(NPOW_ERR_HIP, "injected launch failure (NANOPOW_FAULT_HIP)");
  // Sweep jobs: this launch's set of hit records (PoolHits) starts from zero counts, in stream order.  Its previous
  // user, the launch before the last, has retired -- at most two are in flight -- and its hits were read then.
  if (!collect_.empty())
    HIPTRY(hipMemsetAsync(&d_.pst->hits[r & 1], 0, offsetof(PoolHits, rec), d_.stream));  // (n, claim, best, moves)
  if (n <= (uint32_t)kArgEntries) {
    HIPTRY(hipEventRecord(d_.ev_start[r], d_.stream));
    HIPTRY(launch_pool_arg(d_.stream, sh.grid, t, bounded, d_.pst, d_.pmb_dev));
  } else {
    HIPTRY(hipMemcpyAsync(d_.d_tab[r], d_.h_tab[r], bytes, hipMemcpyHostToDevice, d_.stream));
    HIPTRY(hipEventRecord(d_.ev_start[r], d_.stream));
    HIPTRY(launch_pool(d_.stream, sh.grid, d_.d_tab[r], bounded, d_.pst, d_.pmb_dev));
  }
  // The set's counters come back in stream order right behind the launch, into the ring's own pinned copy: they are
  // there when the stop event fires.  (Copied on the copy stream once the launch had retired, as the records still
  // are, the worker waited for a copy that ran only when a compute unit had room -- beside a launch whose workgroups
  // all hash, as a shared job's moves make them, at that launch's end: every early finish and adoption waited with it.)
  if (!collect_.empty())
    HIPTRY(hipMemcpyAsync(d_.h_hit_ring + (size_t)r * (offsetof(PoolHits, rec) / sizeof(unsigned long long)),
                          &d_.pst->hits[r & 1], offsetof(PoolHits, rec), hipMemcpyDeviceToHost, d_.stream));
  HIPTRY(hipEventRecord(d_.ev_stop[r], d_.stream));
  if (q_.empty()) front_start_ = std::chrono::steady_clock::now();
  NPOW_DBGT("nanopow[%d]: launch %llu n=%u linger %u wsum %u (weights halved %u times) yield_base %llx slots:", d_.id,
            (unsigned long long)seq_, n, t.linger, t.wsum ? t.wsum : pool_claimed_pad_sum(t.pad), t.wdown, (unsigned long long)t.yield_base);
  for (uint32_t e = 0; e < n; ++e) NPOW_DBG(" %d/g%llu", idx[e], (unsigned long long)t.e[e].gen);
  NPOW_DBG("\n");
  q_.push_back({seq_, r, (uint32_t)ctl_, t.yield_base, t.counted != 0, t.linger != 0, t.wdown, bounded, collect_});
  publish_counted();
  return NPOW_OK;
}

// Slots that just left the tables: read their done shards back in stream order, behind every
// launch that still holds them (later launches do not), and note when that copy lands.  Round 5: a won or killed
// slot's kernels publish its final count (every launch, one-entry ones included), so the read-back -- a copy on the
// stream between the dying launch and the next search's launch, ~GPU idle on every device each search -- waits for
// that record: a slot finished from it is freed without a read-back once its launches have completed (every
// kVerifyEvery-th still reads back and checks), and the read-back runs only when no record came (the launches ended
// first: a kill that no poll relayed before the budget ran out; a bounded range exhausted; an invalid win).
int Worker::queue_readbacks() {
  constexpr size_t row = kPoolDoneShards * 8;
  DEVCHECK(d_, "pool read-back");
  for (int s = 0; s < kMaxSlots; ++s) {
    Slot& sl = slots_[s];
    if (sl.state != SlotState::kDraining || sl.readback || sl.no_readback) continue;
    if (!g_readback_always && !d_.dead) {
      if (sl.early) {
        if (++early_count_ % kVerifyEvery != 0) {
          sl.no_readback = true;
          continue;
        }
      } else if (!sl.fin_seen && sl.stop_us > 0 && !sl.requeue && !sl.inflight.empty() &&
                 now_us() - sl.stop_us < g_linger_us) {
        continue;  // won or killed: its final count is on the way (or its launches end without one) -- for
                   // g_linger_us at most: then the read-back is queued now, before the next launch is issued
                   // (ADVICE r05), not behind it; a final count that still comes is checked against it (retire_slots())
      }
    }
    HIPTRY(hipMemcpyAsync(d_.h_done + (size_t)s * row, &d_.pst->done[s][0], row * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, d_.stream));
    HIPTRY(hipEventRecord(d_.ev_done[s], d_.stream));
    sl.readback = true;
  }
  return NPOW_OK;
}

// NANOPOW_TRACE_LATENCY: retired launch f's event span against its clock waves' span g0..g1 (dispatch and drain), and
// the GPU timeline of each decided job it held, from the deciding win (the same clock only for devices on one GPU: CU
// partitions)
void Worker::trace_launch(const PoolInflight& f, uint64_t g0, uint64_t g1) {
  float ev = 0.f;
  if (hipEventElapsedTime(&ev, d_.ev_start[f.ring], d_.ev_stop[f.ring]) == hipSuccess)
    fprintf(stderr, "nanopow-launch dev %d launch %llu: events %.1f clock waves %.1f us, start %.1f us after the "
            "previous end\n", d_.id, (unsigned long long)f.seq, ev * 1e3, (double)(g1 - g0) / 100.0,
            prev_g1_ ? ((double)g0 - (double)prev_g1_) / 100.0 : -1.0);
  prev_g1_ = g1;
  for (const Slot& sl : slots_)
    if (sl.state != SlotState::kFree && sl.job && sl.job->gpu_t_win && !sl.inflight.empty() &&
        sl.inflight.front().seq <= f.seq)
      fprintf(stderr, "nanopow-gpu dev %d ticket %llu launch %llu: start %+.1f end %+.1f us from the win\n", d_.id,
              (unsigned long long)sl.job->ticket, (unsigned long long)f.seq,
              ((double)g0 - (double)sl.job->gpu_t_win) / 100.0, ((double)g1 - (double)sl.job->gpu_t_win) / 100.0);
}

// NANOPOW_TRACE_LATENCY: slot s's decided job stopped on this device when launch seq ended, with no final count
void Worker::trace_nofin(int s, uint64_t seq) const {
  fprintf(stderr, "nanopow-nofin dev %d ticket %llu slot %d g%llu: stopped at its launch's end, no final "
          "count (launch %llu, fin gen %llu)\n", d_.id, (unsigned long long)slots_[s].job->ticket, s,
          (unsigned long long)slots_[s].gen, (unsigned long long)seq,
          (unsigned long long)__atomic_load_n(&d_.pmb->fin[s].gen, __ATOMIC_ACQUIRE));
}

// Launch f has completed: the hits of its collecting entries (sweep jobs) go to their jobs.  The set's counters, then
// each entry's records up to its count or its region's end, are copied on the device's copy stream (not the launch
// stream: the next launch may be running on it) into pinned memory; the launch after next, which zeroes this set
// again, is issued only after this returns.  A count above the region means records were lost (JobDev::hits_lost;
// collect_span makes that a once-in-10^15 event); the job keeps its first NPOW_SWEEP_JOB_HITS hits per device, in
// ascending order -- a device's launches take its part's ranges in that order -- and counts them all.
int Worker::collect_hits(const PoolInflight& f) {
  if (f.collect.empty()) return NPOW_OK;
  DEVCHECK(d_, "pool hit read-back");
  PoolHits* set = &d_.pst->hits[f.ring & 1];
  static_assert(offsetof(PoolHits, claim) == sizeof(PoolHits::n) && offsetof(PoolHits, moves) == 3 * sizeof(PoolHits::n) &&
                    offsetof(PoolHits, rec) == 4 * sizeof(PoolHits::n),
                "the hit and claim counters (and the best words and move counters behind them) are read with one copy");
  // (the counters: the launch's own copy, made in stream order behind it -- Worker::launch)
  memcpy(d_.h_hit_n, d_.h_hit_ring + (size_t)f.ring * (offsetof(PoolHits, rec) / sizeof(unsigned long long)),
         offsetof(PoolHits, rec));
  for (const PoolInflight::Collect& c : f.collect) {
    Slot& sl = slots_[c.slot];
    if (sl.state == SlotState::kFree || sl.gen != c.gen) continue;  // (a slot keeps its job while a launch holds it)
    const uint64_t n = d_.h_hit_n[c.slot];
    const uint64_t stored = std::min<uint64_t>(n, c.room);
    if (stored) {
      HIPTRY(hipMemcpyAsync(d_.h_hits, set->rec + (size_t)c.region * c.room, stored * sizeof(uint64_t),
                            hipMemcpyDeviceToHost, d_.hit_stream));
      HIPTRY(hipStreamSynchronize(d_.hit_stream));
    }
    if (sl.job->is_best()) collect_best(sl, c, f, n, stored);
    else collect_sweep(sl, c, f, n, stored);
  }
  return NPOW_OK;
}

// A best job's entry c of a retired launch, its `stored` records in d_.h_hits (collect_hits): the nonces that beat the
// launch's best as their waves came (ls2_best), the span's maximum among them.  Each value is recomputed here, on the
// CPU, and nothing else of the record is trusted; a nonce outside the entry's span, or more records than the region
// holds (n > stored: the maximum may be among the lost ones), fails the job -- it never returns a possibly wrong
// answer.
void Worker::collect_best(Slot& sl, const PoolInflight::Collect& c, const PoolInflight& f, uint64_t n,
                          uint64_t stored) {
  Job& j = *sl.job;
  std::vector<uint64_t> values(stored);
  bool outside = false;
  for (uint64_t i = 0; i < stored; ++i) {
    outside = outside || d_.h_hits[i] - c.base >= c.count;
    values[i] = host_work_value(j.pre.m, d_.h_hits[i]);
  }
  std::lock_guard<std::mutex> g(g_pool.mu);
  JobDev& jd = j.dev[sl.k];
  jd.hit_n += n;
  jd.launches++;
  if (c.claim) jd.moves += d_.h_hit_n[3 * kMaxSlots + c.slot];  // (PoolHits::moves, read with the counters)
  j.best.records += n;
  j.best.records_max = std::max(j.best.records_max, n);
  j.best.room = j.best.room ? std::min<uint64_t>(j.best.room, c.room) : c.room;
  if ((outside || n > stored) && !j.decided) {
    j.err = "best job: device " + std::to_string(d_.id) +
            (outside ? " recorded a nonce outside its launch's span"
                     : " appended " + std::to_string(n) + " records where its region holds " + std::to_string(c.room));
    decide_locked(j, NPOW_ERR_INTERNAL);
    g_pool.decisions.fetch_add(1, std::memory_order_release);
    notify_workers_locked();
    return;
  }
  // (the records of a launch that was cut are folded like any: the next table's entry carries best_watch of them)
  const uint64_t floor = j.threshold.load(std::memory_order_relaxed);
  for (uint64_t i = 0; i < stored && !outside; ++i) best_fold(j.best.of, j.start, floor, d_.h_hits[i], values[i]);
  credit_entry(sl, c, f);
}

// What retired launch f covered of collecting entry c's span is credited to its job (caller holds g_pool.mu): all of
// it -- or, a claimed entry (a background job's), the first `claims` chunks, claim_prefix(c.count, claims) nonces
// (npow_claims.h); the rest goes back to the front of the device's queue of ranges, in range order (credit_launch,
// npow_credit.h), and the slot is offered to the next table.  Nothing is credited once the slot's generation has stopped (a cancel: its launches ended part-way; the
// done counts' read-back tells what was hashed).  Sweep jobs and best jobs alike.
void Worker::credit_entry(Slot& sl, const PoolInflight::Collect& c, const PoolInflight& f) {
  Job& j = *sl.job;
  JobDev& jd = j.dev[sl.k];
  if (sl.stop_us > 0 || j.decided.load()) return;
  const LaunchCredit cr =
      credit_launch(jd.todo, j.start, c.base, c.count, c.claim, c.claim ? d_.h_hit_n[kMaxSlots + c.slot] : 0);
  if (c.claim) {
    sl.claimed += cr.covered;
    for (Slot::Issued& r : sl.inflight)
      if (r.seq == f.seq && r.base == c.base) r.count = cr.covered;
    if (cr.cut) {
      jd.launches_cut++;
      sl.no_more = false;
    }
  }
  jd.progress += cr.covered;
}

// A sweep job's entry c of retired launch f, its `stored` records in d_.h_hits (collect_hits): the hits go to the
// job's list of this device, in range order.
void Worker::collect_sweep(Slot& sl, const PoolInflight::Collect& c, const PoolInflight& f, uint64_t n,
                           uint64_t stored) {
  const uint64_t start = sl.job->start;
  std::sort(d_.h_hits, d_.h_hits + stored, [start](uint64_t x, uint64_t y) { return x - start < y - start; });
  std::lock_guard<std::mutex> g(g_pool.mu);
  JobDev& jd = sl.job->dev[sl.k];
  jd.hit_n += n;
  if (n > stored) jd.hits_lost = true;
  const uint64_t take = std::min<uint64_t>(stored, (uint64_t)NPOW_SWEEP_JOB_HITS - jd.hits.size());
  jd.hits.insert(jd.hits.end(), d_.h_hits, d_.h_hits + take);
  jd.launches++;
  if (c.claim) jd.moves += d_.h_hit_n[3 * kMaxSlots + c.slot];  // (PoolHits::moves, read with the counters)
  credit_entry(sl, c, f);
}

// The launches that have completed, in order: their statistics, and the ranges they held leave the slots' inflight.
int Worker::retire_launches() {
  while (!q_.empty()) {
    const PoolInflight f = q_.front();
    const hipError_t e = hipEventQuery(d_.ev_stop[f.ring]);
    if (e == hipErrorNotReady) break;
    if (e != hipSuccess) return fail(NPOW_ERR_HIP, std::string("pool launch: ") + hipGetErrorString(e));
    account_launch(d_, f.ring);
    // the GPU idle before this launch: the previous launch's stop event to this one's start event (the ring slot of
    // the previous launch is not reused before this one retires: at most two launches are in flight)
    if (prev_stop_ring_ >= 0) {
      float gap = 0.f;
      if (hipEventElapsedTime(&gap, d_.ev_stop[prev_stop_ring_], d_.ev_start[f.ring]) == hipSuccess && gap >= 0.f)
        stat([&] { d_.idle_ms += gap; d_.idle_gaps++; });
    }
    prev_stop_ring_ = f.ring;
    uint64_t g0 = 0, g1 = 0;
    account_clock(f.ring, f.seq, &g0, &g1);
    if (g_trace_lat && g0) trace_launch(f, g0, g1);
    if (int rc = collect_hits(f)) return rc;  // sweep jobs: before their slots can retire (retire_slots)
    // The launch's ranges are complete, except those of a generation that won in it (or in an
    // earlier launch still unseen): handle such wins first, they hand back what did not finish.
    for (int s = 0; s < kMaxSlots; ++s) {
      Slot& sl = slots_[s];
      if (sl.state == SlotState::kFree || sl.inflight.empty()) continue;
      if (win_published(s)) handle_win(s);
      size_t m = 0;
      while (m < sl.inflight.size() && sl.inflight[m].seq <= f.seq) ++m;
      // dense bounded ranges, hashed in full (fail_all's accounting) -- unless the slot's generation has
      // stopped (won or killed): its launches may have ended part-way, so nothing more is credited
      if (sl.job && sl.job->max_per_dev && !sl.win_seen && sl.stop_us == 0)
        for (size_t i = 0; i < m; ++i) sl.unread += sl.inflight[i].count;
      sl.inflight.erase(sl.inflight.begin(), sl.inflight.begin() + (ptrdiff_t)m);
      if (sl.inflight.empty()) sl.ending = false;
      // a decided job's last launch on this device has completed: the device hashes nothing more of it, so
      // its stop time is now (npow_wait_info), not when the done counts' read-back lands
      // (a slot finished from its final count has its stop time already: no pool lock for it -- a lingering launch
      // retires with up to 33 of them, and 33 acquisitions of the contended lock held up this worker's next look at
      // a live search by up to ~0.1 ms)
      if (m > 0 && sl.inflight.empty() && sl.state == SlotState::kDraining && !sl.early && sl.job &&
          sl.job->decided.load()) {
        std::lock_guard<std::mutex> g(g_pool.mu);
        JobDev& jd = sl.job->dev[sl.k];
        if (jd.t_stop == 0) {
          jd.t_stop = now_us();
          if (g_trace_lat) trace_nofin(s, f.seq);
        }
      }
    }
    if (g_trace_lat)
      for (Slot& sl : slots_)
        if (sl.state == SlotState::kDraining && sl.job && sl.job->t_win != 0 && sl.job->t_kend == 0)
          sl.job->t_kend = now_us();
    NPOW_DBGT("nanopow[%d]: launch %llu done\n", d_.id, (unsigned long long)f.seq);
    retired_seq_ = f.seq;
    q_.pop_front();
    publish_counted();
    front_start_ = std::chrono::steady_clock::now();  // the next one (if any) has just started
  }
  return NPOW_OK;
}

// The draining slots that no launch holds any more: their counts go to their jobs, which leave the device, are
// handed back for re-adoption, or (a dropped device) go to the survivors; the slots are freed.
int Worker::retire_slots() {
  constexpr size_t row = kPoolDoneShards * 8;
  for (int s = 0; s < kMaxSlots; ++s) {
    Slot& sl = slots_[s];
    if (sl.state == SlotState::kDraining && sl.no_readback && sl.inflight.empty()) {
      // finished from its published final count and every launch that held it has completed: nothing can still add
      // to its done counts, so the next job of this slot starts from the published total (sl.baseline)
      free_slot(s);
      continue;
    }
    if (sl.state != SlotState::kDraining || !sl.readback) continue;
    // a sweep job's slot retires only after retire_launches() has read the hits of every launch that held it (the
    // read-back's event may fire between that call's look at the launch's event and this one)
    if (sl.job->collects() && !sl.inflight.empty()) continue;
    const hipError_t e = hipEventQuery(d_.ev_done[s]);
    if (e == hipErrorNotReady) continue;
    if (e != hipSuccess) return fail(NPOW_ERR_HIP, std::string("pool read-back: ") + hipGetErrorString(e));
    // every launch that held the slot has completed: its done shards are final
    uint64_t sum = 0, late = 0, stale_hits = 0;
    for (int i = 0; i < kPoolDoneShards; ++i) {
      sum += d_.h_done[(size_t)s * row + i * 8];
      late += d_.h_done[(size_t)s * row + i * 8 + kLateWord];
      stale_hits += d_.h_done[(size_t)s * row + i * 8 + kStaleWord];
    }
    const Counts c = credit_counts(sl, sum, late, stale_hits);  // (c.stale: 0 for a slot finished from its final count)
    if (win_published(s)) handle_win(s);  // published by the last launch, not yet seen
    if (sl.stale && !sl.fin_seen) {  // every launch that held it has ended: its count came late, or never
      if (__atomic_load_n(&d_.pmb->fin[s].gen, __ATOMIC_ACQUIRE) == sl.gen) {
        uint64_t tw = 0;
        {
          std::lock_guard<std::mutex> g(g_pool.mu);
          tw = sl.job ? sl.job->gpu_t_win : 0;
        }
        stale_fin_came(s, tw);
      } else {
        stat([&] { d_.stale_missing++; });
      }
    }
    NPOW_DBG("nanopow[%d]: retire slot %d g%llu done %llu requeue %d early %d\n", d_.id, s,
             (unsigned long long)sl.gen, (unsigned long long)c.done, (int)sl.requeue, (int)sl.early);
    if (sl.early) {  // finished by early_finish(): the read-back must add nothing to its count
      if (c.done != 0) {
        fprintf(stderr, "nanopow: GPU %d slot %d: read back %llu nonces past the published final count\n", d_.id,
                s, (unsigned long long)c.done);
        std::lock_guard<std::mutex> sg(d_.stats_mu);
        d_.early_mismatch++;
      }
    } else {
      std::lock_guard<std::mutex> g(g_pool.mu);
      Job& j = *sl.job;
      credit_job_locked(sl, c);
      if (j.claimed() && !j.decided && !d_.dead && c.done != sl.claimed) {
        // a claimed job: the nonces its workgroups counted are not the prefixes its launches' claims covered
        j.err = std::string(j.shared ? "shared" : "background") + (j.is_best() ? " best job" : " sweep job") + ": device " +
                std::to_string(d_.id) + " hashed " + std::to_string(c.done) +
                " nonces where its claims cover " + std::to_string(sl.claimed);
        decide_locked(j, NPOW_ERR_INTERNAL);
        g_pool.decisions.fetch_add(1, std::memory_order_release);
        notify_workers_locked();
      }
      if (d_.dead) {
        abandon_locked(sl.job, sl.k, d_.dead_code, d_.dead_msg);  // survivors take what is left
      } else if (!j.decided && (sl.requeue || !j.dev[sl.k].todo.empty())) {
        j.dev[sl.k].on = false;  // adopt() picks it up again with a fresh generation
        g_pool.version.fetch_add(1);
      } else {
        device_done_locked(sl.job, sl.k);
      }
    }
    free_slot(s);
  }
  return NPOW_OK;
}

// A HIP call failed: the device is dropped at once (no draining: its queue cannot be trusted).
// Ranges of launches that had not completed go back to their jobs, which re-stride them.
void Worker::fail_all(const std::string& msg) {
  fprintf(stderr, "nanopow: device %d failed: %s; dropping it\n", d_.id, msg.c_str());
  std::lock_guard<std::mutex> g(g_pool.mu);
  if (!d_.dead) drop(NPOW_ERR_HIP, "device " + std::to_string(d_.id) + " failed: " + msg);
  for (int s = 0; s < kMaxSlots; ++s) {
    Slot& sl = slots_[s];
    if (sl.state == SlotState::kFree) continue;
    if (sl.job->max_per_dev) {
      // no read-back from a failed device: the job counts its bounded ranges that completed here
      // (each hashed in full, dense) from their sizes; the rest go back to it and are re-strided.
      // Exact for a job that ends without a hit; once the slot's generation has stopped (a win, a kill)
      // its last launches may have ended part-way, so only the ranges retired before that are counted
      // (crediting them in full over-counted a won job): a lower bound then.
      const uint64_t kept = push_back_locked(sl, 0, true);
      const bool stopped = sl.win_seen || sl.stop_us > 0;
      if (!sl.early) sl.job->done += sl.unread + (stopped ? 0 : kept);
    }
    const JobP j = sl.job;
    free_slot(s);  // disarmed before the job can end (abandon_locked): the watcher reads its cancel word
    abandon_locked(j, sl.k, d_.dead_code, d_.dead_msg);
  }
  q_.clear();
  prev_stop_ring_ = -1;
}

int Worker::step() {
  timed(0, [&] { adopt(); return 0; });
  timed(1, [&] { check_slots(); return 0; });
  if (!q_.empty() && !live_slot()) {
    // a lingering launch idle for g_linger_us, or something waiting for the device, or its time budget over.  Idle
    // means also no won or killed slot still draining in it (its final count not in): ended under such a slot, the
    // launch's yield would race the kill relay (npow_kernel.hip ls2_poll).  A slot whose final count has not come
    // g_linger_us after its stop no longer holds the launch (stale): its count then comes from the launch's completion
    // and the read-back -- rare (1 search in ~1,200 over 4 CU partitions, profiles/r05aj_linger_by_partition_overshoot
    // .jsonl), but without this bound the lingering launch ran on to its budget and the stop took 21 ms.
    const double t = now_us();
    bool draining = false, stale = false, lingering = false;
    for (const PoolInflight& f : q_) lingering = lingering || f.linger;
    for (Slot& sl : slots_) {
      if (sl.state != SlotState::kDraining || sl.fin_seen || sl.inflight.empty()) continue;
      // (the record read again after t: a worker descheduled for a millisecond between check_slots' look and here
      // would otherwise count a count that came meanwhile as stale -- round 6 saw 8 at once over 8 partitions)
      if (sl.stop_us > 0 && t - sl.stop_us > g_linger_us &&
          __atomic_load_n(&d_.pmb->fin[&sl - slots_].gen, __ATOMIC_ACQUIRE) != sl.gen) {
        stale = true;
        if (!sl.stale && lingering) {  // the fallback below fires for it: counted, and classified when the slot's count
                                       // comes late or not at all (early_finish / retire_slots: stale_missing)
          sl.stale = true;
          std::lock_guard<std::mutex> sg(d_.stats_mu);
          d_.stale_drains++;
          NPOW_DBGT("nanopow[%d]: slot %d g%llu: no final count %.0f us after its stop\n", d_.id,
                    (int)(&sl - slots_), (unsigned long long)sl.gen, t - sl.stop_us);
        }
      } else {
        draining = true;
      }
    }
    if (idle_since_ == 0 && !draining) idle_since_ = t;
    // the GPU time a lingering launch spends waiting with nothing to hash (its HIP-event time includes it):
    // npow_device_stats.linger_ms, so that kernel_ms - linger_ms is the time the device hashed
    if (lingering && !draining && q_.front().linger) {
      if (linger_t_ > 0) stat([&] { d_.linger_ms += (t - linger_t_) * 1e-3; });
      linger_t_ = t;
    } else {
      linger_t_ = 0;
    }
    bool waiting = d_.tasks_waiting.load() > 0 || d_.dead || g_pool.stopping.load(std::memory_order_relaxed) ||
                   (stale && !draining) || (idle_since_ > 0 && t - idle_since_ > g_linger_us) || budget_left_us() < 0;
    for (int s = 0; s < kMaxSlots && !waiting; ++s) waiting = slots_[s].state == SlotState::kActive;  // (fresh)
    if (waiting) {
      end_linger();
    } else if (!draining && q_.size() == 1 && q_.front().linger && d_.tasks_waiting.load() == 0 &&
               (uint32_t)((uint32_t)ctl_ - (uint32_t)q_.front().dyn_base) >= (uint32_t)kDynEntries) {
      // idle, and its dynamic entries used up: the next search could not join it, and would wait for it to end and
      // for a launch of its own (0.1-0.7 ms over 8 CU partitions, every 33rd search of a serial client).  End it now
      // and queue an empty lingering launch behind it, whose workgroups take the CUs as its own leave; the next
      // search joins that one (dyn_add), in ring positions the ending launch does not read.
      end_linger();
      if (int rc = timed(3, [&] { return launch(true); })) return rc;
    }
  } else {
    idle_since_ = 0;
    linger_t_ = 0;
  }
  if (int rc = timed(2, [&] { return queue_readbacks(); })) return rc;  // before the next launch: it no longer holds them
  if (d_.tasks_waiting.load() == 0)                                       // a sweep / values call is waiting: drain instead
    if (int rc = timed(3, [&] { return launch(); })) return rc;
  if (int rc = timed(4, [&] { return retire(); })) return rc;
  publish_busy();
  return NPOW_OK;
}

void Worker::run() {
  prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);  // nap(): 1-us timer slack instead of the default 50 us
  t_pool_worker = true;
  if (hipSetDevice(d_.hip_id) != hipSuccess)
    drop(NPOW_ERR_HIP, "device " + std::to_string(d_.id) + ": hipSetDevice failed");
  struct OnExit {
    const Worker& w;
    ~OnExit() {
      if (g_trace_steps) w.print_prof();
    }
  } on_exit{*this};
  for (;;) {
    if (exit_now()) return;
    if (d_.dead && !busy()) {
      // a dropped device (drained) hands every job that still names it to that job's survivors
      if (dev_lock_.owns_lock()) dev_lock_.unlock();
      std::unique_lock<std::mutex> lk(g_pool.mu);
      for (const JobP& j : std::vector<JobP>(g_pool.active)) {
        const int k = index_in(*j, d_.id);
        if (k >= 0 && !j->dev[k].done) abandon_locked(j, (size_t)k, d_.dead_code, d_.dead_msg);
      }
      if (!g_pool.running) return;
      g_pool.cv_work.wait(lk);
      continue;
    }
    if (!busy()) adopt();  // jobs admitted since the last look
    if (!busy()) {
      publish_busy();
      if (dev_lock_.owns_lock()) dev_lock_.unlock();
      // Spin a little before sleeping: a serial client submits its next request a few tens of
      // microseconds after the last one ends, and a condition-variable wake-up costs about as
      // much as the search itself at receive difficulty.
      const auto spin_end = std::chrono::steady_clock::now() + std::chrono::microseconds(kIdleSpinUs);
      while (g_pool.version.load(std::memory_order_acquire) == seen_version_ &&
             !exit_now() && d_.tasks_waiting.load() == 0 &&
             std::chrono::steady_clock::now() < spin_end)
        cpu_relax();
      if (g_pool.version.load(std::memory_order_acquire) != seen_version_) continue;
      std::unique_lock<std::mutex> lk(g_pool.mu);
      g_pool.cv_work.wait(lk, [&] { return !g_pool.running || wants_device_locked(d_.id); });
      if (!g_pool.running) return;
      continue;
    }
    if (d_.tasks_waiting.load() > 0 && q_.empty()) {
      // hand the device to a waiting sweep / values call (TaskLock); lock() below then waits
      // for it to finish
      prev_stop_ring_ = -1;  // the task records the device's events too
      if (dev_lock_.owns_lock()) dev_lock_.unlock();
      while (d_.tasks_waiting.load() > 0 && !exit_now())
        std::this_thread::sleep_for(std::chrono::microseconds(50));
      continue;
    }
    if (!dev_lock_.owns_lock()) dev_lock_.lock();  // waits behind a sweep / values task on this device
    int rc;
    try {
      rc = step();
    } catch (const std::exception& e) {  // nothing may leave the worker thread
      rc = fail(NPOW_ERR_INTERNAL, std::string("pool worker: ") + e.what());
    }
    if (rc != NPOW_OK) {
      fail_all(last_error());
      if (dev_lock_.owns_lock()) dev_lock_.unlock();
      continue;
    }
    timed(5, [&] { nap(); return 0; });
  }
}

// Between two steps.  While a launch runs there is nothing to do until a win is published, a
// job is decided or cancelled, new jobs arrive (they notify cv_work) or the next launch must be
// queued: poll without sleeping only during the first kFreshSpinUs of a launch (wins at receive
// difficulty come that early) and near the next launch's queueing point; otherwise sleep up to
// g_poll_us on cv_work.  A win is then seen within ~g_poll_us and the thread uses ~6 % of a core
// instead of all of it (50 us: 27.13 Gnonce/s on the serial bench vs 27.07 spinning, 26.98 at
// 200 us; profiles/r02_ab_worker_nap.txt).
void Worker::nap() {
  if (g_poll_us <= 0 || q_.empty() || d_.dead || d_.tasks_waiting.load() > 0) {
    cpu_relax();
    return;
  }
  // a won / killed slot drains within a hash or two (~20-40 us): poll until its count is in, for at
  // most kStopSpinUs after the stop
  const double t = now_us();
  for (const Slot& sl : slots_)
    if (sl.state == SlotState::kDraining && sl.stop_us > 0 && !sl.fin_seen && t - sl.stop_us < kStopSpinUs) {
      cpu_relax();
      return;
    }
  const double since = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - front_start_).count();
  if (since < kFreshSpinUs) {
    cpu_relax();
    return;
  }
  double us = g_poll_us;
  const double budget = (double)g_budget_us.load();
  if (q_.size() == 1 && budget > 0) {
    const double until_prelaunch = budget - kPrelaunchUs - since;
    if (until_prelaunch <= 0) {
      cpu_relax();
      return;
    }
    us = std::min(us, until_prelaunch);
  }
  // on the device's own condition variable (round 5): new jobs, decisions and shutdown bump wake_seq
  // (notify_workers_locked); one that came since the last nap returns at once
  std::unique_lock<std::mutex> wl(d_.wake_mu);
  d_.wake_cv.wait_for(wl, std::chrono::duration<double, std::micro>(us),
                      [&] { return d_.wake_seq != wake_seen_ || d_.tasks_waiting.load() > 0; });
  wake_seen_ = d_.wake_seq;
}

}  // namespace

// -- device resources -----------------------------------------------------------------------------
int pool_device_init(Device& d) {
  DEVCHECK(d, "pool_device_init");
  HIPTRY(hipMalloc(&d.pst, sizeof(PoolDevState)));
  if (int rc = check_device_memory(d.pst, d, "the pool state")) return rc;
  // on the device's own stream, not the null stream: a CU-partitioned device's stream is a blocking one
  HIPTRY(hipMemsetAsync(d.pst, 0, sizeof(PoolDevState), d.stream));
  HIPTRY(hipStreamSynchronize(d.stream));
  void* mb = nullptr;
  HIPTRY(hipHostMalloc(&mb, sizeof(PoolMailbox), hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable));
  memset(mb, 0, sizeof(PoolMailbox));
  d.pmb = (PoolMailbox*)mb;
  void* mbd = nullptr;  // taken with d.hip_id current (init_device), checked against the allocation's own mapping
  HIPTRY(hipHostGetDevicePointer(&mbd, mb, 0));
  d.pmb_dev = (PoolMailbox*)mbd;
  if (int rc = check_pinned_mapping(mb, mbd, "the pool mailbox")) return rc;
  for (int r = 0; r < kEventRing; ++r) {
    HIPTRY(hipMalloc(&d.d_tab[r], sizeof(PoolTable)));
    if (int rc = check_device_memory(d.d_tab[r], d, "a launch table")) return rc;
    void* h = nullptr;
    HIPTRY(hipHostMalloc(&h, sizeof(PoolTable), hipHostMallocDefault));
    memset(h, 0, sizeof(PoolTable));
    d.h_tab[r] = (PoolTable*)h;
  }
  void* hd = nullptr;
  HIPTRY(hipHostMalloc(&hd, (size_t)kMaxSlots * kPoolDoneShards * 8 * sizeof(unsigned long long), hipHostMallocDefault));
  d.h_done = (unsigned long long*)hd;
  for (int s = 0; s < kMaxSlots; ++s) HIPTRY(hipEventCreateWithFlags(&d.ev_done[s], hipEventDisableTiming));
  // sweep jobs: the copy stream and the pinned staging of a launch's hits (8 MiB; the records themselves are the
  // last 16 MiB of PoolDevState)
  HIPTRY(hipStreamCreateWithFlags(&d.hit_stream, hipStreamNonBlocking));
  void* hn = nullptr;
  HIPTRY(hipHostMalloc(&hn, offsetof(PoolHits, rec) + (size_t)kSweepHits * sizeof(uint64_t), hipHostMallocDefault));
  d.h_hit_n = (unsigned long long*)hn;  // (the hit counters, then the claim counters)
  d.h_hits = (uint64_t*)((char*)hn + offsetof(PoolHits, rec));
  void* hr = nullptr;
  HIPTRY(hipHostMalloc(&hr, (size_t)kEventRing * offsetof(PoolHits, rec), hipHostMallocDefault));
  memset(hr, 0, (size_t)kEventRing * offsetof(PoolHits, rec));
  d.h_hit_ring = (unsigned long long*)hr;
  return NPOW_OK;
}

void pool_device_free(Device& d) {  // tolerates a partial pool_device_init
  if (d.pst) (void)hipFree(d.pst);
  if (d.pmb) (void)hipHostFree(d.pmb);
  for (int r = 0; r < kEventRing; ++r) {
    if (d.d_tab[r]) (void)hipFree(d.d_tab[r]);
    if (d.h_tab[r]) (void)hipHostFree(d.h_tab[r]);
  }
  if (d.h_done) (void)hipHostFree(d.h_done);
  for (int s = 0; s < kMaxSlots; ++s)
    if (d.ev_done[s]) (void)hipEventDestroy(d.ev_done[s]);
  if (d.h_hit_n) (void)hipHostFree(d.h_hit_n);  // (h_hits is part of it)
  if (d.h_hit_ring) (void)hipHostFree(d.h_hit_ring);
  if (d.hit_stream) (void)hipStreamDestroy(d.hit_stream);
}

void pool_start() {
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    g_pool.running = true;
    g_pool.stopping = false;
  }
  watch_start();
  for (auto& dp : g_devs) {
    Device* d = dp.get();
    if (d->cpu_threads) {
      d->worker = std::thread([d] { cpu_worker_run(*d); });
      continue;
    }
    d->worker = std::thread([d] {
      Worker w(*d);
      w.run();
    });
  }
}

// Process exit (npow_init's atexit hook).  Round 6: the workers used to leave at once, without a HIP
// call, and a lingering launch (up to its 20-ms budget of waiting, polling pinned memory) or a search launch could
// still be running while the HIP runtime and a profiler's tool library tore down -- the process then died with SIGSEGV
// in its exit handlers under rocprofv3 (profiles/r05aq_hip_api_trace_overshoot_g4.txt).  Now exit drains like
// npow_shutdown: every job is cancelled (its kill word raised), lingering launches get their yield, the workers retire
// their launches and leave once idle -- for up to kExitDrainMs; after that (a device that does not answer) they leave
// regardless.  The hook runs before the HIP runtime's own exit handlers (it was registered after the runtime was
// loaded and initialised: atexit runs in reverse order), so the workers' HIP calls (event queries) are still valid.
constexpr double kExitDrainMs = 250.0;
bool pool_exit() {
  g_exit_deadline_us.store(now_us() + kExitDrainMs * 1e3);
  pool_stop();
  const bool drained = !g_exiting.load();  // (set only by exit_now() once the deadline passed)
  g_exiting = true;
  return drained;
}

void pool_stop() {
  {
    std::lock_guard<std::mutex> g(g_pool.mu);
    g_pool.running = false;
    g_pool.stopping = true;  // workers end their lingering launches (end_linger)
    for (const JobP& j : g_pool.active) j->cancel_req = true;
    notify_workers_locked();
  }
  for (auto& d : g_devs)
    if (d->worker.joinable()) d->worker.join();
  watch_stop();
  std::lock_guard<std::mutex> g(g_pool.mu);
  for (auto& kv : g_pool.tickets) {
    const JobP& j = kv.second;
    if (!j->finished) {
      if (!j->decided) {  // a decided job keeps its outcome: waiters may read it without the lock
        j->err = "engine shut down";
        j->status = NPOW_ERR_NOT_INITIALISED;
        j->decided.store(true, std::memory_order_release);
      }
      j->finished.store(true, std::memory_order_release);
    }
  }
  for (auto& kv : g_pool.tickets) notify_waiters(*kv.second);
  g_pool.waiting.clear();
  g_pool.active.clear();
}

}  // namespace npow
