// npow_pool.h -- the work pool's jobs and their state transitions (npow_pool.cpp), shared by the GPU workers, the
// ticket calls (npow_pool_jobs.cpp), the win watcher (npow_pool_watch.cpp) and the CPU workers (npow_cpu.cpp,
// `--cpu-threads`).
// Internal to libnanopow.so.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "npow_best.h"
#include "npow_credit.h"
#include "npow_host.h"

namespace npow {

constexpr int kPending = 100;  // job status before it is decided
inline double now_us() {       // steady clock, microseconds
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// (Range -- [base, base + count) mod 2^64, nonces of a job still to be handed to launches -- is npow_credit.h's)

// A job's state on the k-th of its devices (Job::dev[k]; guarded by g_pool.mu)
struct JobDev {
  std::deque<Range> todo;  // ranges not yet handed to a launch (a dead device's remainder is re-strided onto the
                           // survivors')
  bool on = false;         // a slot holds the job
  bool seen = false;       // adopted at least once (re-adoptions do not yield)
  bool done = false;       // finished with the job
  int slot = -1;           // the slot holding it while `on` (-1: none; the CPU device has none) ...
  uint64_t gen = 0;        // ... and its generation there (the decider raises their kill words)
  uint64_t res_seen = 0;   // the nonce of the slot's reserve record at the last harvest of this generation, and ...
  uint64_t res_seen_gen = 0;  // ... that generation (pool_harvest_locked validates a record once)
  double t_stop = 0;       // when its worker saw it stop hashing the job (us; 0 = never adopted)
  double t_launch = 0;     // when its first launch holding the job was issued (us; 0 = none)
  uint64_t late = 0;       // nonces its waves hashed after they knew the job was over (device-side count,
                           // PoolDevState kLateWord)
  // A sweep job's hits on this device (Worker::collect_hits, as each launch that held its entry retires): the
  // nonces, ascending by (nonce - Job::start), at most NPOW_SWEEP_JOB_HITS of them -- the first ones, while no
  // launch's records overflowed (hits_lost) -- and their exact number.
  std::vector<uint64_t> hits;
  uint64_t hit_n = 0;
  bool hits_lost = false;
  // What npow_ticket_sweep, npow_ticket_best and npow_ticket_best_hold report of a collecting job on this device
  // (Worker::credit_entry, Worker::hold_out).
  // progress: the nonces the retired launches covered (a launch's whole span; of a background job's launch the prefix
  // its claims covered, npow_claims.h).  launches_cut: launches of a background job that ended with part of their span
  // unhashed (a yield, the time budget).  held_us / held_since: how long the job's slot was left out of this device's
  // tables because a foreground job wanted the device, and since when it is (0 = it is not).
  uint64_t progress = 0, launches = 0, launches_cut = 0;
  double held_us = 0, held_since = 0;
  uint64_t moves = 0;  // workgroups that came to the job's claimed entries from another entry of a running launch (the
                       // kernel's count, PoolHits::moves, summed over the retired launches; npow_ticket_share)
};

enum class JobKind : uint8_t { kSearch, kSweep, kBest };

struct Job {
  uint64_t ticket = 0;
  RootPrecomp pre{};
  uint64_t u[NPOW_ASM_N_UNIFORMS] = {};
  std::atomic<uint64_t> threshold{0};  // written under g_pool.mu (the submit; pool_retarget raises it, pool_relax
                                       // lowers it, never below `reserve`); the win watcher, the GPU workers and the
                                       // CPU workers read it without the lock
  // Reserve hits (npow_submit_reserve; all guarded by g_pool.mu).  reserve: the reserve threshold, <= threshold at the
  // submit; equal to it for every other submit (not armed): such a job's entries, waves and records are as before.
  uint64_t reserve = 0;
  bool armed = false;               // reserve < threshold at the submit
  uint64_t res_nonce = 0, res_value = 0;  // the best reserve validated so far (pool_harvest_locked); value 0 = none
  int res_dev = -1;                 // the logical device whose record held it
  bool answered = false;            // pool_relax decided the job from its reserve
  uint64_t relaxes = 0;             // lowerings of the threshold that took effect (pool_relax)
  uint64_t candidates = 0;          // reserve records read from the GPUs and validated
  // The job's kind (set at the submit, never changes: read without the lock).  A search (pool_submit) is decided by
  // its first win.
  // A sweep job (npow_submit_sweep): a bounded job (max_per_dev != 0: its devices' largest part) that never wins --
  // its entries collect every hit of [start, start + count) (PoolEntry::bounded kEntryCollect, JobDev::hits), each
  // device a contiguous part.  Only pool_wait_sweep collects its ticket; a part is never handed to another device.
  // A best job (npow_submit_best): a sweep job's sibling whose entries keep only what beats the
  // best value so far (PoolEntry::bounded kEntryBest).  Same admission, parts, range queues and retirement; its
  // launches' few records are validated on the CPU and folded into `best.of` as they retire (Worker::collect_best,
  // npow_best.h), and each new entry carries best_watch() as its threshold.  `threshold` holds the floor.  Only
  // pool_wait_best collects its ticket.
  // Either collecting kind with `background` set (npow_submit_sweep_background, npow_submit_best_background; it never
  // changes: npow_promote refuses the ticket) is a claimed job: its entries are claimed ones (kEntryClaim, beside
  // kEntryBest for a best job) and a device leaves its slot out of every table built while a foreground job is live
  // there (Worker::hold_out).
  // Either collecting kind with `shared` set (npow_submit_sweep_shared, npow_submit_best_shared; it never changes) is
  // a claimed job too, but a foreground one that no table leaves out: it weighs 1 in the start map of a table whose
  // bounded entries are all claimed (pool_table_weights_claimed), and its entries take the workgroups that the searches
  // of its launch no longer want (npow_kernel.hip ls2_move_claimed).  `background` stays false.
  JobKind kind = JobKind::kSearch;
  bool collects() const { return kind != JobKind::kSearch; }  // its entries collect records: a sweep or a best job
  bool is_best() const { return kind == JobKind::kBest; }
  bool claimed() const { return collects() && (background || shared); }  // its entries are claimed ones
  bool held_class() const { return collects() && background; }  // a collecting job of the background class (hold_out)
  int range_class() const { return background ? 1 : shared ? 2 : 0; }  // npow_range_share_info::klass
  struct Best {  // a best job's own state (guarded by g_pool.mu)
    BestFold of;
    uint64_t records = 0;      // records read from its retired launches, and ...
    uint64_t records_max = 0;  // ... the most one launch's entry appended (npow_ticket_best)
    uint64_t room = 0;         // the smallest region one of its entries had (records; 0 = no launch yet)
  } best;
  uint64_t count = 0;
  uint64_t start = 0, max_per_dev = 0, spacing = 0;
  const volatile uint32_t* cancel = nullptr;
  uint32_t weight = 1;    // 1, 2, 4 or 8 (npow_submit_weighted): its share of each GPU's workgroups among the live
                          // unbounded jobs, and its place in the admission queue; the CPU device ignores it
  bool background = false;  // npow_submit_background, until npow_promote lifts it (guarded by g_pool.mu): each GPU
                            // hashes it only on workgroups no foreground job wants (PoolEntry::bg), and it is admitted
                            // behind every foreground job; weight stays 1 meanwhile.  The CPU device ignores it
  bool shared = false;      // a collecting job of the shared class (above); set at the submit, never changes
  std::vector<int> devs;  // device ids; the k-th starts on [start + k * spacing, + stride)
  std::vector<JobDev> dev;  // per device k of devs; guarded by g_pool.mu
  uint64_t retargets = 0;           // raises of the threshold that took effect (pool_retarget)
  uint64_t stale_hits = 0;          // lanes the devices' waves refused: below the slot's floor (kStaleWord)
  uint64_t stale_wins = 0;          // wins published under an older threshold, refused and re-armed (Worker::handle_win)
  int winner_k = -1;                // the device whose result decided the job
  int pending_devs = 0;
  std::atomic<bool> admitted{false};  // written under g_pool.mu; waiters read it without it
  bool lost = false;                // a dead device's remainder had no surviving device to go to
  int lost_code = NPOW_ERR_HIP;
  std::atomic<bool> finished{false};  // written under g_pool.mu; waiters may spin on it
  // Its waiters (pool_wait, pool_wait_result) sleep on cv with wmu, not g_pool.mu (round 5): a waiter woken at the
  // decision then returns without queueing for the pool lock behind the workers that the same decision woke (over 8
  // devices that convoy cost ~25 us per search, profiles/r05a_regime8_new.json).  decide_locked / finish_locked lock
  // wmu before they notify, and a job's outcome (status, nonce, value, err) is written before `decided` is
  // released and never after it, so a waiter reads it once it has acquired `decided`.
  std::mutex wmu;
  std::condition_variable cv;
  int status = kPending;
  uint64_t nonce = 0, value = 0, done = 0;
  std::string err;
  // lock-free flags the workers poll
  std::atomic<bool> decided{false};
  std::atomic<bool> cancel_req{false};

  bool cancel_seen() const { return cancel_req.load(std::memory_order_relaxed) || (cancel && load_acquire(cancel)); }
  // host timestamps of the job's life (steady clock, us): npow_wait_info reports them (t_kend only for
  // NANOPOW_TRACE_LATENCY, which prints the timeline in pool_wait).  t_win: the first win record read; t_win_seen:
  // the deciding one (CPU re-validation then decides at t_decide)
  double t_submit = 0, t_adopt = 0, t_launch = 0, t_win = 0, t_kend = 0, t_finish = 0, t_decide = 0, t_win_seen = 0;
  uint64_t gpu_t_win = 0;  // the deciding win's s_memrealtime (PoolWin::t; NANOPOW_TRACE_LATENCY GPU timelines)
  double spin_us = 2000.0;  // how long its result waiters and the win watcher poll before they sleep
                            // (npow_pool_watch.cpp spin_window_us: ~3 x its expected time to a win, in [2, 50] ms)
};
using JobP = std::shared_ptr<Job>;

struct Pool {
  std::mutex mu;
  std::condition_variable cv_work;  // idle workers: new admissions / shutdown (busy ones nap on their device's wake_cv)
  std::deque<JobP> waiting;
  std::vector<JobP> active;
  std::unordered_map<uint64_t, JobP> tickets;
  uint64_t next_ticket = 1;
  uint32_t max_active = kMaxSlots;
  bool running = false;
  std::atomic<bool> stopping{false};  // pool_stop: workers end their lingering launches at once
  std::atomic<uint64_t> version{0};  // bumped whenever `active` gains a job
  std::atomic<uint64_t> decisions{0};  // bumped when a job split over devices is decided: wakes napping workers
};
extern Pool g_pool;  // npow_pool.cpp

extern std::atomic<uint64_t> g_gen;      // slot generations (unique, > 0)
extern std::atomic<bool> g_exiting;      // process exit, drain over (or its deadline passed): workers leave at once
// Process exit (pool_exit, round 6): the workers drain their launches like pool_stop until this deadline (steady clock
// us; 0 = not exiting), then leave.  exit_now(): the deadline has passed (it then sets g_exiting) or g_exiting is set.
extern std::atomic<double> g_exit_deadline_us;
inline bool exit_now() {
  if (g_exiting.load(std::memory_order_relaxed)) return true;
  const double d = g_exit_deadline_us.load(std::memory_order_relaxed);
  if (d > 0 && now_us() > d) {
    g_exiting.store(true);
    return true;
  }
  return false;
}

// The pool lock with its notifications deferred (round 6): the waiters' condition variables and the
// workers' wakes that decide_locked / finish_locked / stop_other_devices_locked / admit_locked make under it are sent
// after the lock is released, not while it is held.  Each is a futex wake-up; made under the lock, the woken thread
// may preempt the holder on its CPU, and every other thread wanting the lock (the losing devices' workers publishing
// their stop) then waits for the holder to be scheduled again.  Use it only where every job decided or finished under
// it stays referenced past its scope (a slot's or a local JobP): the deferred list holds plain pointers.
class PoolLock {
 public:
  PoolLock();
  ~PoolLock();
  PoolLock(const PoolLock&) = delete;
  PoolLock& operator=(const PoolLock&) = delete;

 private:
  std::unique_lock<std::mutex> lk_;
};

// -- job state transitions (caller holds g_pool.mu; npow_pool.cpp) ------------------------------
void decide_locked(Job& j, int status, uint64_t nonce = 0, uint64_t value = 0);
void admit_locked();
// A job's rank in the waiting queue (heaviest first, FIFO within a rank): its weight, background jobs behind all
inline uint32_t queue_rank(const Job& j) { return j.background ? 0u : j.weight; }
void finish_locked(const JobP& j);
// t_seen: when the device's worker observed it stop hashing the job (its final count read), 0 = now
void device_done_locked(const JobP& j, size_t k, double t_seen = 0.0);
void abandon_locked(const JobP& j, size_t k, int code, const std::string& msg);
void stop_other_devices_locked(Job& j, size_t k_win);
// Device k's result (nonce, value), re-validated by the caller and not below the job's threshold, decides job j,
// which is still pending: the outcome, the timestamps, the winner, and the other devices' kill words.  t_seen: when the
// win record was read, gpu_t: its PoolWin::t (both 0 for the CPU device, which has no record).
void accept_win(Job& j, size_t k, uint64_t nonce, uint64_t value, double t_seen, uint64_t gpu_t);
inline int index_in(const Job& j, int dev) {  // the job's index of logical device dev, or -1
  for (size_t k = 0; k < j.devs.size(); ++k)
    if (j.devs[k] == dev) return (int)k;
  return -1;
}
void notify_workers_locked();         // wake the idle workers (cv_work) and the napping ones (each device's wake_cv)
bool wants_device_locked(int dev);    // some active job wants this device

// -- CPU workers (npow_cpu.cpp) ------------------------------------------------------------------
void cpu_worker_run(Device& d);  // the pool worker of a CPU device (Device::cpu_threads > 0)

}  // namespace npow
