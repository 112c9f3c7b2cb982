// npow_pool_watch.cpp -- the work pool's win watcher.
//
// A device's pool worker sees its winner records only between its naps (up to g_poll_us = 50 us once a launch is
// 0.4 ms old), and over 8 devices a worker woken by a notify queues for the pool lock behind the others.  One thread
// for the whole process instead spins over the win records of every armed slot of every GPU while any job is live
// (one core; it reads pinned host memory only, no HIP call), re-validates a winner on the CPU and decides the job
// at once: the result goes to the client and the other devices' kill words go up within microseconds of the
// record landing.  The winner's worker handles the same record at its next step as before (an invalid result, the
// device's invalid streak and the slot's retirement stay its business; a job already decided is left alone).
// It also watches each armed job's cancel word (a caller's work_cancel, or another rank's first win through a shared
// word, bench.py node_time_to_work) and wakes the device's worker at once, which then stops the job's waves.
// Spinning is bounded (round 6): the watcher spins while a job armed on a slot is within its spin window
// -- three times the job's expected time to a win at its devices' rate (a win comes in it with probability 0.95),
// at least kWatchSpinUs, at most kWatchSpinMaxUs; kWatchSpinUs only when a CPU device's hashing threads share the host
// (--cpu-threads) -- or within kWatchSpinUs of a record it handled, and otherwise naps g_watch_nap_us at a time (1-us
// timer slack).  So an endless or very hard search, or an idle lingering launch, costs a fraction of a core instead of
// all of it, while a search of the expected length (the serial client's, 2-15 ms at fffffff8 on 8 GPUs or on one)
// is watched spinning: a flat 2-ms window had put the nap's delay (~10-15 us) on every search longer than 2 ms -- the
// 8-GPU time regime's fixed cost per search 6 -> 16 us on one GPU (profiles/r06f_regime1.json).
// NANOPOW_WATCH_NAP_US=0 spins always.
#include <sys/prctl.h>

#include <algorithm>
#include <chrono>
#include <thread>

#include "npow_pool_impl.h"

namespace npow {
namespace {
constexpr double kWatchSpinUs = 2000.0;
constexpr double kWatchSpinMaxUs = 50000.0;
constexpr double kNoncesPerCuUs = 139.0;  // a CU's search rate (35.6 Gnonce/s over 256 CUs)
struct Watch {
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<int> armed{0};        // armed slots over all devices
  std::atomic<uint64_t> arms{0};    // arms so far (a new one restarts the spin window)
  bool stop = false;
  std::thread th;
};
Watch g_watch;
}  // namespace

// The slot's spin window (above): 3 x the job's expected nonces to a win / its GPU devices' rate, in [2, 50] ms.
double spin_window_us(const Job& j) {
  bool cpu_device = false;
  double rate = 0.0;  // nonces per us
  for (const auto& dp : g_devs) cpu_device = cpu_device || dp->cpu_threads > 0;
  if (cpu_device) return kWatchSpinUs;
  for (int id : j.devs) {
    const Device& d = *g_devs[(size_t)id];
    if (!d.cpu_threads) rate += d.cus * kNoncesPerCuUs;
  }
  const double expect = 18446744073709551616.0 / (18446744073709551616.0 - (double)j.threshold.load() + 1.0);
  const double w = rate > 0 ? 3.0 * expect / rate : kWatchSpinMaxUs;
  return std::min(kWatchSpinMaxUs, std::max(kWatchSpinUs, w));
}

void watch_arm(Device& d, int s, uint64_t gen, const JobP& j) {
  if (!g_watcher_on) return;
  d.armed_spin_until[s].store(now_us() + j->spin_us, std::memory_order_relaxed);
  {
    std::lock_guard<std::mutex> g(d.armed_mu);
    d.armed_job[s] = j;
  }
  d.armed_cancel[s].store(j->cancel, std::memory_order_release);
  d.armed_gen[s].store(gen, std::memory_order_release);
  const uint64_t bit = 1ull << s;
  g_watch.arms.fetch_add(1, std::memory_order_acq_rel);  // (a napping watcher sees it within its nap: no wake-up here,
                                                         // under the pool lock; a win comes ~0.2 ms after an arm at best)
  if (!(d.armed_mask.fetch_or(bit, std::memory_order_acq_rel) & bit) &&
      g_watch.armed.fetch_add(1, std::memory_order_acq_rel) == 0) {
    { std::lock_guard<std::mutex> g(g_watch.mu); }
    g_watch.cv.notify_one();
  }
}

void watch_disarm(Device& d, int s) {
  if (!g_watcher_on) return;
  const uint64_t bit = 1ull << s;
  if (d.armed_mask.fetch_and(~bit, std::memory_order_acq_rel) & bit) g_watch.armed.fetch_sub(1, std::memory_order_acq_rel);
  std::lock_guard<std::mutex> g(d.armed_mu);  // (see watch_stop_cancel)
  d.armed_gen[s].store(0, std::memory_order_release);
  d.armed_cancel[s].store(nullptr, std::memory_order_release);
  d.armed_job[s].reset();
}

// The slot leaves the searching state: the watcher stops reading its job's cancel word.  Under armed_mu, which the
// watcher holds while it reads the word: the device cannot finish with the job before this, so the job cannot end and
// its caller free the word while the watcher reads it.
void watch_stop_cancel(Device& d, int s) {
  if (!g_watcher_on) return;
  std::lock_guard<std::mutex> g(d.armed_mu);
  d.armed_cancel[s].store(nullptr, std::memory_order_release);
}

namespace {
void watch_handle(Device& d, int s, uint64_t gen) {
  const double t_seen = now_us();
  JobP j;
  {
    std::lock_guard<std::mutex> g(d.armed_mu);
    if (d.armed_gen[s].load(std::memory_order_acquire) == gen) j = std::static_pointer_cast<Job>(d.armed_job[s]);
  }
  if (!j) return;
  uint64_t n, v;
  read_win(d, s, &n, &v);
  if (__atomic_load_n(&d.pmb->win[s].gen, __ATOMIC_ACQUIRE) != gen) return;  // the record moved on meanwhile
  if (host_work_value(j->pre.m, n) != v || v < j->threshold.load(std::memory_order_relaxed))
    return;  // invalid, or below a raised threshold (npow_retarget): the worker's business
  PoolLock g;  // (j, a local reference, outlives it)
  const int k = index_in(*j, d.id);
  if (j->status != kPending || k < 0 || j->dev[(size_t)k].gen != gen) return;
  if (v < j->threshold.load(std::memory_order_relaxed)) return;  // raised since the look above (pool_retarget holds
                                                                 // this lock): a decision never undercuts a raise
  accept_win(*j, (size_t)k, n, v, t_seen, __atomic_load_n(&d.pmb->win[s].t, __ATOMIC_RELAXED));
  if (j->devs.size() < 2) notify_workers_locked();  // (stop_other_devices_locked wakes them for split jobs)
  std::lock_guard<std::mutex> sg(d.stats_mu);
  d.watcher_decisions++;
}

void watcher_run() {
  prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
  std::vector<std::vector<uint64_t>> handled(g_devs.size(), std::vector<uint64_t>(kMaxSlots, 0));
  std::vector<std::vector<uint64_t>> cancelled(g_devs.size(), std::vector<uint64_t>(kMaxSlots, 0));
  uint64_t arms_seen = g_watch.arms.load(std::memory_order_acquire);
  double t_event = now_us();  // the last arm or record change: spin until kWatchSpinUs after it
  for (uint32_t round = 0;; ++round) {
    if (g_watch.armed.load(std::memory_order_acquire) == 0) {
      std::unique_lock<std::mutex> lk(g_watch.mu);
      g_watch.cv.wait(lk, [] { return g_watch.stop || g_watch.armed.load(std::memory_order_acquire) > 0; });
      if (g_watch.stop) return;
      t_event = now_us();
    }
    if (exit_now()) return;
    if ((round & 63u) == 0) {  // (the clock every 64 rounds: a round over a few armed slots is ~0.1 us)
      const uint64_t a = g_watch.arms.load(std::memory_order_acquire);
      const double t = now_us();
      double until = t_event + kWatchSpinUs;  // the armed slots' spin windows (watch_arm)
      for (const auto& dp : g_devs) {
        for (uint64_t m = dp->armed_mask.load(std::memory_order_acquire); m; m &= m - 1)
          until = std::max(until, dp->armed_spin_until[__builtin_ctzll(m)].load(std::memory_order_relaxed));
      }
      if (a != arms_seen) {
        arms_seen = a;
      } else if (g_watch_nap_us > 0 && t > until) {
        std::unique_lock<std::mutex> lk(g_watch.mu);
        g_watch.cv.wait_for(lk, std::chrono::duration<double, std::micro>(g_watch_nap_us), [&] {
          return g_watch.stop || g_watch.arms.load(std::memory_order_acquire) != arms_seen;
        });
        if (g_watch.stop) return;
      }
    }
    for (size_t di = 0; di < g_devs.size(); ++di) {
      Device& d = *g_devs[di];
      uint64_t m = d.armed_mask.load(std::memory_order_acquire);
      while (m) {
        const int s = __builtin_ctzll(m);
        m &= m - 1;
        const uint64_t gen = d.armed_gen[s].load(std::memory_order_acquire);
        if (gen && gen != handled[di][s] && __atomic_load_n(&d.pmb->win[s].gen, __ATOMIC_ACQUIRE) == gen) {
          handled[di][s] = gen;
          watch_handle(d, s, gen);
          t_event = now_us();
        }
        if (gen && gen != cancelled[di][s] && d.armed_cancel[s].load(std::memory_order_acquire)) {
          bool raised;
          {
            std::lock_guard<std::mutex> g(d.armed_mu);  // (watch_stop_cancel)
            const volatile uint32_t* c = d.armed_cancel[s].load(std::memory_order_acquire);
            raised = c && load_acquire(c);
          }
          if (raised) {
            cancelled[di][s] = gen;
            wake_worker(d);  // its check_slots sees the cancel word and raises the slot's kill word
          }
        }
      }
    }
    cpu_relax();
  }
}
}  // namespace

void watch_start() {
  if (!g_watcher_on) return;
  {
    std::lock_guard<std::mutex> g(g_watch.mu);
    g_watch.stop = false;
  }
  g_watch.th = std::thread(watcher_run);
}

void watch_stop() {
  if (g_watch.th.joinable()) {
    {
      std::lock_guard<std::mutex> g(g_watch.mu);
      g_watch.stop = true;
    }
    g_watch.cv.notify_all();
    g_watch.th.join();
  }
  for (auto& dp : g_devs)  // a worker that left with slots armed (shutdown): nothing is watched any more
    for (int s = 0; s < kMaxSlots; ++s) watch_disarm(*dp, s);
}

}  // namespace npow
