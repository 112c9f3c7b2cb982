// npow_pool_jobs.cpp -- the work pool's ticket calls, the functions behind the C ABI's job calls (npow_engine.cpp):
// the submits, the waits, the looks at a ticket and the calls that change a live job (cancel, promote, retarget,
// relax).  Each finds its job by the ticket, refuses a ticket of another kind (expect_kind), and works under the pool
// lock alone -- none waits for a GPU.  npow_pool.cpp has the state transitions they call and the workers that act on
// what they write.
//
// A job has one of three kinds (Job::kind):
// A search (npow_submit and its variants) is decided by its first win; pool_wait_result returns at the decision,
// pool_wait collects the ticket.  Its threshold can move while it runs (pool_retarget, pool_relax).
// A sweep job (npow_submit_sweep) is a bounded job that never wins: its entries collect every hit of their ranges in
// the launch's hit records (PoolHits), which the worker reads as each launch retires (Worker::collect_hits);
// pool_wait_sweep merges them.  DESIGN.md section 1 "Sweep jobs".  With Job::background
// (npow_submit_sweep_background) the workers leave it out of a device's tables while a foreground job is live there.
// DESIGN.md section 1 "Background sweep jobs".
// A best job (npow_submit_best) is a sweep job whose entries (kEntryBest) keep only the nonces that beat
// the best value their launch has seen; the workers fold them into the job's best (Worker::collect_best), and
// pool_wait_best returns it.  DESIGN.md section 1 "Best jobs".  With Job::background (npow_submit_best_background) it
// is of the background sweep job's class, claimed entries and all.  DESIGN.md section 1 "Background best jobs".
// Either collecting kind with Job::shared (npow_submit_sweep_shared, npow_submit_best_shared) is a foreground job with
// claimed entries that is never held out; pool_ticket_share tells the class.  DESIGN.md section 1 "Shared range jobs".
#include <algorithm>

#include "npow_pool_impl.h"

namespace npow {
namespace {

// -- what every ticket call shares -------------------------------------------------------------------
// The job of a ticket (caller holds g_pool.mu), or null: the call then fails with "unknown ticket".
JobP ticket_job_locked(uint64_t ticket) {
  auto it = g_pool.tickets.find(ticket);
  if (it != g_pool.tickets.end()) return it->second;
  fail(NPOW_ERR_BAD_ARGUMENT, "unknown ticket");
  return nullptr;
}
// ... for the waits, which hold the lock for the lookup only
JobP ticket_job(uint64_t ticket) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  return ticket_job_locked(ticket);
}

// A ticket is collected by its own kind's wait and cancelled by pool_cancel; every call of another kind is
// refused and leaves the job as it was (Job::kind does not change after the submit: no lock needed).  The refusal
// names the ticket's kind and, in parentheses, the wait that collects it -- or, `look` (npow_ticket_sweep), the look
// of its kind, which a search has none of.
constexpr const char* kKindWords[3][3] = {  // the ticket's kind: whose it is, its collecting wait, its look
    {"a search's", " (npow_wait collects it)", ""},
    {"a sweep job's", " (npow_wait_sweep collects it)", " (npow_ticket_sweep)"},
    {"a best job's", " (npow_wait_best collects it)", " (npow_ticket_best)"}};
int expect_kind(const Job& j, JobKind want, const char* call, bool look = false) {
  if (j.kind == want) return NPOW_OK;
  const char* const* w = kKindWords[(size_t)j.kind];
  return fail(NPOW_ERR_BAD_ARGUMENT, std::string(call) + ": the ticket is " + w[0] + w[look ? 2 : 1]);
}

// Job j's place in the waiting queue, which is kept by rank, heaviest first, FIFO within a rank (admit_locked takes
// its front): behind the last job at least as heavy.  With every weight 1 this is the back.  Background jobs rank
// behind all (queue_rank).
void queue_locked(const JobP& j) {
  auto at = g_pool.waiting.end();
  while (at != g_pool.waiting.begin() && queue_rank(**(at - 1)) < queue_rank(*j)) --at;
  g_pool.waiting.insert(at, j);
}

// A new job gets its ticket and, unless it was complete at the submit (an empty range), its place in the queue.
int enqueue_locked(const JobP& j, uint64_t* ticket) {
  if (!g_pool.running) return fail(NPOW_ERR_NOT_INITIALISED, "engine is shut down");
  j->ticket = g_pool.next_ticket++;
  g_pool.tickets[j->ticket] = j;
  if (!j->finished) {
    queue_locked(j);
    admit_locked();
  }
  *ticket = j->ticket;
  return NPOW_OK;
}

// -- waiting ---------------------------------------------------------------------------------------------
// Waiters of a search's outcome (npow_wait_result) poll instead of sleeping while at most kMaxSpinners of them do,
// for up to the job's spin window per call (Job::spin_us: ~3 x its expected time to a win, 2-50 ms; 2 ms beside CPU
// workers): a serial client's reply then leaves as soon as the job is decided instead of after a condition-variable
// wake-up (decided -> result in the client p50 11 -> 6 us), and a search far longer than
// expected -- or one nobody expects to end -- is waited for asleep (round 6, ADVICE r05: a flat 50 ms before).
// NANOPOW_WAIT_SPIN=0 turns it off (A/B runs).
constexpr int kMaxSpinners = 2;
std::atomic<int> g_spinners{0};

// Wait, without g_pool.mu, until done() holds (NPOW_OK) or the timeout passes (NPOW_PENDING).  A queued job's
// cancel word is polled here every 2 ms (admitted ones are polled by the device workers), and such a job is cancelled
// under the pool lock.  spin: poll first (g_spinners above).
template <class Done>
int wait_job(const JobP& j, int64_t timeout_us, Done done, bool spin = false) {
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(timeout_us < 0 ? 0 : timeout_us);
  if (spin && g_wait_spin && timeout_us != 0) {
    if (g_spinners.fetch_add(1, std::memory_order_relaxed) < kMaxSpinners) {
      const int64_t spin_us = (int64_t)j->spin_us;
      const auto spin_end = std::chrono::steady_clock::now() +
                            std::chrono::microseconds(timeout_us < 0 ? spin_us : std::min(timeout_us, spin_us));
      for (uint32_t k = 0; !done(); ++k) {
        cpu_relax();
        if ((k & 255u) == 0 && (std::chrono::steady_clock::now() >= spin_end ||
                                (!j->admitted.load(std::memory_order_acquire) && j->cancel_seen())))
          break;
      }
    }
    g_spinners.fetch_sub(1, std::memory_order_relaxed);
  }
  for (;;) {
    if (done()) return NPOW_OK;
    if (!j->admitted.load(std::memory_order_acquire) && j->cancel_seen()) {
      std::lock_guard<std::mutex> g(g_pool.mu);
      if (!j->admitted && !j->finished) {
        j->cancel_req = true;
        decide_locked(*j, NPOW_CANCELLED);
        finish_locked(j);
      }
      continue;
    }
    const auto now = std::chrono::steady_clock::now();
    if (timeout_us >= 0 && now >= deadline) return NPOW_PENDING;
    std::unique_lock<std::mutex> wl(j->wmu);
    if (j->admitted.load(std::memory_order_acquire) && timeout_us < 0) {
      j->cv.wait(wl, done);
    } else {
      auto wake = j->admitted.load(std::memory_order_acquire) ? deadline : now + std::chrono::microseconds(2000);
      if (timeout_us >= 0) wake = std::min(wake, deadline);
      j->cv.wait_until(wl, wake, done);
    }
  }
}

// ... until the job has finished on all its devices: what the collecting waits wait for
int wait_finished(const JobP& j, int64_t timeout_us) {
  return wait_job(j, timeout_us, [&] { return j->finished.load(std::memory_order_acquire); });
}

// A decided job's outcome as pool_wait and pool_wait_result return it.
int outcome(const Job& j, uint64_t* nonce, uint64_t* value) {
  const int st = j.status;
  if (st == NPOW_OK) {
    if (nonce) *nonce = j.nonce;
    if (value) *value = j.value;
  }
  return st < 0 ? fail(st, j.err.empty() ? std::string("work generation failed") : j.err) : st;
}

// -- what the collecting waits share (pool_wait_sweep, pool_wait_best) ------------------------------------------------
// A job that has ended and whose ticket is released: its outcome as it stood under the pool lock.
struct Ended {
  JobP job;
  int status = kPending;
  uint64_t done = 0;
  std::string err;
  int hashed_all(const char* what) const {  // a job that was not cancelled hashed its whole range, or it fails
    if (status == NPOW_CANCELLED || done == job->count) return NPOW_OK;
    return fail(NPOW_ERR_INTERNAL, std::string(what) + ": hashed " + std::to_string(done) + " nonces of " +
                                       std::to_string(job->count));
  }
};

// Wait until the ticket's job, of kind `want`, has finished on all its devices, release the ticket and copy its
// outcome -- and whatever snapshot(job) reads of it -- under the pool lock.  NPOW_OK, or what the call returns at
// once: NPOW_PENDING (the ticket stays), or the refusal of an unknown ticket or one of another kind.
template <class Snapshot>
int wait_ended(uint64_t ticket, JobKind want, const char* call, int64_t timeout_us, Ended* e, Snapshot snapshot) {
  e->job = ticket_job(ticket);
  if (!e->job) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*e->job, want, call)) return rc;
  if (wait_finished(e->job, timeout_us) == NPOW_PENDING) return NPOW_PENDING;
  std::lock_guard<std::mutex> g(g_pool.mu);
  g_pool.tickets.erase(ticket);
  snapshot(*e->job);
  e->status = e->job->status;
  e->done = e->job->done;
  e->err = e->job->err;
  return NPOW_OK;
}

}  // namespace

// -- searches ----------------------------------------------------------------------------------------
int pool_submit(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t device_mask,
                uint64_t max_nonces_per_device, const volatile uint32_t* cancel, uint64_t* ticket, uint32_t weight,
                bool background, uint64_t reserve) {
  // A bounded search over "all devices" (mask 0) leaves the CPU workers out: their stride would be as
  // long as a GPU's at ~1/1000 of its rate, nothing hands their leftover to an idle GPU, and they work on one job
  // at a time -- an exhausting search would wait for them.  An explicit mask may still name the CPU device.
  auto devs = max_nonces_per_device && device_mask == 0 ? select_gpus(0) : select_devices(device_mask);
  if (devs.empty() && max_nonces_per_device && device_mask == 0) devs = select_devices(0);  // only the CPU is left
  if (devs.empty()) return fail(NPOW_ERR_NO_DEVICE, "no usable device in device_mask");
  auto j = std::make_shared<Job>();
  j->pre = host_precompute(root);
  npow_asm_uniforms(j->pre.m, j->u);
  j->threshold = threshold;
  j->armed = reserve < threshold && !max_nonces_per_device;
  j->reserve = j->armed ? reserve : threshold;
  j->start = start;
  j->max_per_dev = max_nonces_per_device;
  j->cancel = cancel;
  j->weight = max_nonces_per_device ? 1u : weight;
  j->background = background && !max_nonces_per_device;
  const uint64_t G = devs.size();
  j->spacing = G > 1 ? (~0ull / G) + 1 : 0;  // 2^64 / G (exact for powers of two)
  for (Device* d : devs) j->devs.push_back(d->id);
  j->dev.resize(G);
  for (uint64_t k = 0; k < G; ++k) {
    // bounded: max_nonces_per_device; unbounded: the whole stride (2^64 / G; 2^64 - 1 with one device)
    const uint64_t cnt = max_nonces_per_device ? max_nonces_per_device : (G > 1 ? j->spacing : ~0ull);
    j->dev[k].todo.push_back({start + k * j->spacing, cnt});
  }
  j->pending_devs = (int)G;
  j->spin_us = spin_window_us(*j);
  j->t_submit = now_us();
  std::lock_guard<std::mutex> g(g_pool.mu);
  return enqueue_locked(j, ticket);
}

int pool_wait(uint64_t ticket, int64_t timeout_us, uint64_t* nonce, uint64_t* value, uint64_t* nonces_done,
              npow_search_info* info) {
  JobP j = ticket_job(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*j, JobKind::kSearch, "npow_wait")) return rc;
  if (wait_finished(j, timeout_us) == NPOW_PENDING) return NPOW_PENDING;
  std::unique_lock<std::mutex> lk(g_pool.mu);
  if (nonces_done) *nonces_done = j->done;
  if (info) {
    info->winner_device = j->winner_k >= 0 ? j->devs[(size_t)j->winner_k] : -1;
    info->n_devices = (int32_t)j->devs.size();
    info->decide_us = j->t_decide > 0 ? j->t_decide - j->t_submit : 0.0;
    info->finish_us = j->t_finish - j->t_submit;
    double worst = 0.0, over = 0.0;
    if (j->t_decide > 0)
      for (size_t k = 0; k < j->devs.size(); ++k) {
        if ((int)k == j->winner_k || j->dev[k].t_stop <= j->t_decide) continue;
        const double span = j->dev[k].t_stop - j->t_decide;
        worst = std::max(worst, span);
        Device& d = *g_devs[(size_t)j->devs[k]];
        std::lock_guard<std::mutex> sg(d.stats_mu);
        if (d.kernel_ms > 0) over += span * 1e-3 * (double)d.nonces / d.kernel_ms;  // us x nonces per ms
      }
    info->stop_after_decide_us = worst;
    info->overshoot_nonces = (uint64_t)over;
    uint64_t dev_late = 0;
    for (size_t k = 0; k < j->devs.size(); ++k)
      if ((int)k != j->winner_k) dev_late += j->dev[k].late;
    info->late_nonces_losers = dev_late;
    info->late_nonces_winner = j->winner_k >= 0 ? j->dev[(size_t)j->winner_k].late : 0;
    auto since = [&](double t) { return t > 0 ? t - j->t_submit : 0.0; };
    info->adopt_us = since(j->t_adopt);
    info->launch_us = since(j->t_launch);
    double all = 0.0;
    for (size_t k = 0; k < j->devs.size(); ++k) {
      if (j->dev[k].t_launch == 0) {  // a device that never launched it (decided before it got to it; the CPU device)
        all = 0.0;
        break;
      }
      all = std::max(all, j->dev[k].t_launch);
    }
    info->launch_all_us = since(all);
    info->win_seen_us = since(j->t_win_seen);
    info->retargets = j->retargets;
    info->stale_hits = j->stale_hits;
    info->stale_wins = j->stale_wins;
  }
  if (g_trace_lat) {
    fprintf(stderr, "nanopow-lat adopt %.1f launch %.1f win %.1f kend %.1f finish %.1f return %.1f", j->t_adopt - j->t_submit,
            j->t_launch - j->t_submit, j->t_win - j->t_submit, j->t_kend - j->t_submit, j->t_finish - j->t_submit,
            now_us() - j->t_submit);
    if (j->devs.size() > 1 && j->t_decide > 0) {  // the devices' stop times after the decision
      fprintf(stderr, " decide %.1f stops", j->t_decide - j->t_submit);
      for (size_t k = 0; k < j->devs.size(); ++k)
        fprintf(stderr, " %s%.1f", (int)k == j->winner_k ? "*" : "",
                j->dev[k].t_stop > 0 ? j->dev[k].t_stop - j->t_decide : -1.0);
    }
    fprintf(stderr, "\n");
  }
  g_pool.tickets.erase(ticket);
  return outcome(*j, nonce, value);
}

// The search's outcome as soon as it is known (npow_wait_result): the winner accepted or the job cancelled,
// while the other devices may still be stopping; the ticket stays valid for pool_wait.
int pool_wait_result(uint64_t ticket, int64_t timeout_us, uint64_t* nonce, uint64_t* value) {
  JobP j = ticket_job(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*j, JobKind::kSearch, "npow_wait_result")) return rc;
  if (wait_job(
          j, timeout_us,
          [&] { return j->decided.load(std::memory_order_acquire) || j->finished.load(std::memory_order_acquire); },
          true) == NPOW_PENDING)
    return NPOW_PENDING;
  return outcome(*j, nonce, value);  // written before `decided` was released, and never after it
}

int pool_ticket_background(uint64_t ticket, uint32_t* background) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP j = ticket_job_locked(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*j, JobKind::kSearch, "npow_ticket_background")) return rc;
  *background = j->background ? 1u : 0u;
  return NPOW_OK;
}

int pool_cancel(uint64_t ticket) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP j = ticket_job_locked(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (j->finished) return NPOW_OK;
  j->cancel_req = true;
  if (!j->admitted) {
    decide_locked(*j, NPOW_CANCELLED);
    finish_locked(j);
  } else {
    notify_workers_locked();  // the devices' workers stop its waves at their next step, now rather than after a nap
  }
  return NPOW_OK;
}

// Raise a job's weight (npow_promote; the caller checked the weight).  Only the pool lock, as pool_cancel: nothing
// here waits for a GPU.  A waiting job moves up the admission queue.  An admitted one carries the new weight into
// every later table and dynamic entry, and each GPU that holds it now (a slot and a generation) is told (mb_boost), so
// that a running counted launch rebalances to the new weight without ending.  A launch that does
// not read the counter -- a one-entry one -- or none at all loses nothing: the next table has the weight.
int pool_promote(uint64_t ticket, uint32_t weight) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP j = ticket_job_locked(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*j, JobKind::kSearch, "npow_promote")) return rc;
  if (weight > 1 && j->max_per_dev)
    return fail(NPOW_ERR_BAD_ARGUMENT, "a bounded search (max_nonces_per_device) takes weight 1 only");
  // A background job becomes a foreground job of this weight, whatever the weight: the same steps.  (Admitted, it
  // may take the live foreground jobs past max_active: it holds its slot already.)
  const bool lift = j->background;
  if (j->finished || j->decided || j->cancel_req || (!lift && weight <= j->weight)) return NPOW_OK;
  j->weight = weight;
  j->background = false;
  if (!j->admitted) {
    // its new place in the waiting queue (every job behind its old place ranks below the new weight)
    auto at = std::find(g_pool.waiting.begin(), g_pool.waiting.end(), j);
    if (at != g_pool.waiting.end()) {
      g_pool.waiting.erase(at);
      queue_locked(j);
    }
    if (lift) admit_locked();  // (a foreground job does not wait for the live background ones)
    return NPOW_OK;
  }
  for_each_gpu_slot(*j, [&](size_t, Device& d, JobDev& jd) {
    mb_boost(d, jd.slot, jd.gen, weight);
    // counted as published into a running launch: a counted launch is in flight and the job is in one
    if (d.counted_inflight.load(std::memory_order_acquire) > 0 && jd.t_launch != 0) {
      std::lock_guard<std::mutex> sg(d.stats_mu);
      d.promotions++;
    }
  });
  return NPOW_OK;
}

// Raise a job's threshold (npow_retarget).  Only the pool lock, as pool_promote: nothing here waits for a GPU, and
// the lock orders the raise against every decision (decide_locked is called under it, and the win watcher and
// handle_win compare a win with the threshold under it): once this returns NPOW_OK no result below the threshold
// can be decided.  The field is all a waiting job needs, or one no slot holds yet: every table and dynamic entry
// built from now on carries it, and the CPU workers read it at each check.  For each GPU that holds the job in a
// slot the slot's floor record is written (mb_floor), which a wave of a running launch reads when it has a hit
// -- no launch ends, and the entry keeps its slot, generation, weight and nonce
// position.  A win a wave published before it could see the record is refused by Worker::handle_win (stale_wins).
int pool_retarget(uint64_t ticket, uint64_t threshold) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP j = ticket_job_locked(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*j, JobKind::kSearch, "npow_retarget")) return rc;
  if (threshold <= j->threshold.load(std::memory_order_relaxed)) return NPOW_OK;  // never lowered
  if (j->finished || j->decided || j->cancel_seen()) return NPOW_TOO_LATE;        // its outcome stands
  j->threshold.store(threshold, std::memory_order_release);
  j->retargets++;
  // (Job::spin_us stays as the submit set it: waiters read it without the lock, and a window sized for the old
  // threshold only puts a longer search's waiter and watcher to sleep sooner)
  if (!j->admitted || faults().retarget_blind) return NPOW_OK;
  for_each_gpu_slot(*j, [&](size_t, Device& d, JobDev& jd) { mb_floor(d, jd.slot, jd.gen, threshold); });
  return NPOW_OK;
}

// Read the reserve records of every GPU slot that holds job j (caller holds g_pool.mu; no GPU call: pinned host
// memory).  A record is a hint (PoolReserve): only its nonce is used, and its value is recomputed here, so a torn
// record, or one a slot's earlier generation left, comes out below the reserve threshold and is dropped.  Each
// record is validated once (JobDev::res_seen); the job keeps the best.
static void pool_harvest_locked(Job& j) {
  for_each_gpu_slot(j, [&](size_t k, Device& d, JobDev& jd) {
    const PoolReserve& r = d.pmb->reserve[jd.slot];
    if (__atomic_load_n(&r.gen, __ATOMIC_ACQUIRE) != jd.gen) return;
    const uint64_t n = __atomic_load_n(&r.nonce, __ATOMIC_RELAXED);
    if (jd.res_seen_gen == jd.gen && jd.res_seen == n) return;
    jd.res_seen_gen = jd.gen;
    jd.res_seen = n;
    j.candidates++;
    const uint64_t v = host_work_value(j.pre.m, n);
    if (v >= j.reserve && v > j.res_value) {
      j.res_nonce = n;
      j.res_value = v;
      j.res_dev = j.devs[k];
    }
  });
}

// Decide job j from its reserve (caller holds g_pool.mu; the reserve meets the current threshold): the way a win
// of another device goes -- the outcome is set and its waiters are told before this returns, the kill word of every
// device that holds the job goes up, the finder's included (its waves know of no win), and each worker then retires
// its slot from the final count its launch publishes (check_slots, early_finish).
static void pool_answer_locked(Job& j) {
  const int k = index_in(j, j.res_dev);
  accept_win(j, k >= 0 ? (size_t)k : 0u, j.res_nonce, j.res_value, 0.0, 0);
  j.answered = true;
  if (k >= 0) {
    JobDev& jd = j.dev[(size_t)k];
    Device& d = *g_devs[(size_t)j.devs[(size_t)k]];
    if (jd.on && jd.slot >= 0 && !d.cpu_threads && d.pmb) mb_kill(d, jd.slot, jd.gen);
  }
  g_pool.decisions.fetch_add(1, std::memory_order_release);
  notify_workers_locked();
}

int pool_ticket_reserve(uint64_t ticket, npow_reserve_info* out) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP jp = ticket_job_locked(ticket);
  if (!jp) return NPOW_ERR_BAD_ARGUMENT;
  Job& j = *jp;
  if (int rc = expect_kind(j, JobKind::kSearch, "npow_ticket_reserve")) return rc;
  if (j.armed && !j.decided && !j.finished) pool_harvest_locked(j);
  out->armed = j.armed ? 1u : 0u;
  out->reserve_threshold = j.reserve;
  out->threshold = j.threshold.load(std::memory_order_relaxed);
  out->nonce = j.res_nonce;
  out->value = j.res_value;
  out->device = j.res_value ? j.res_dev : -1;
  out->answered = j.answered ? 1u : 0u;
  out->relaxes = j.relaxes;
  out->candidates = j.candidates;
  return NPOW_OK;
}

// Lower a job's threshold (npow_relax).  Only the pool lock, as pool_retarget: nothing here waits for a GPU, and the
// lock orders the lowering against every decision.  The reserves are harvested first: one that meets the new
// threshold decides the job at once.  Otherwise the field is lowered -- every table and dynamic entry built from now
// on carries it, the CPU workers read it at each check -- and each GPU slot's floor record is rewritten (mb_floor),
// which a wave of a running launch reads when a lane meets its watch threshold: lanes at or above the new threshold
// win from then on.  Then a second harvest: a candidate that was on its way to the pinned record while the first
// one ran (its wave had read the old threshold) has landed or will be seen as a win by a later wave; the one that
// has landed may qualify now.
int pool_relax(uint64_t ticket, uint64_t threshold, uint32_t* answered) {
  JobP j;      // (declared before the lock: the job decided under it stays referenced past the lock's scope)
  PoolLock g;
  j = ticket_job_locked(ticket);
  if (!j) return NPOW_ERR_BAD_ARGUMENT;
  if (int rc = expect_kind(*j, JobKind::kSearch, "npow_relax")) return rc;
  if (!j->armed) return fail(NPOW_ERR_BAD_ARGUMENT, "the search was submitted without a reserve threshold");
  if (threshold < j->reserve) return fail(NPOW_ERR_BAD_ARGUMENT, "below the search's reserve threshold");
  if (j->finished || j->decided || j->cancel_seen()) return NPOW_TOO_LATE;  // its outcome stands
  if (threshold >= j->threshold.load(std::memory_order_relaxed)) return NPOW_OK;
  j->relaxes++;
  pool_harvest_locked(*j);
  if (j->res_value < threshold) {
    j->threshold.store(threshold, std::memory_order_release);
    if (j->admitted)
      for_each_gpu_slot(*j, [&](size_t, Device& d, JobDev& jd) { mb_floor(d, jd.slot, jd.gen, threshold); });
    pool_harvest_locked(*j);
  } else {
    j->threshold.store(threshold, std::memory_order_release);
  }
  if (j->res_value >= threshold) {
    pool_answer_locked(*j);
    *answered = 1;
  }
  return NPOW_OK;
}

// -- sweep jobs (npow_submit_sweep, npow_wait_sweep) ----------------------------------------------------------------
// Every hit of [start, start + count) as a pool job: a bounded job of weight 1 and foreground class whose entries
// collect (PoolEntry::bounded kEntryCollect) instead of winning.  The range is split into contiguous parts over the
// GPUs of the mask, as npow_sweep splits it (a GPU whose part would be empty is left out); each worker reads its
// launches' hits as they retire (collect_hits), and pool_wait_sweep merges the devices' lists.
static int submit_collecting(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t count,
                             uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket, JobKind kind,
                             int klass) {
  auto j = std::make_shared<Job>();
  j->kind = kind;  // (a best job: `threshold` is its floor)
  j->background = klass == 1;  // (npow_submit_sweep_background, npow_submit_best_background: admitted as a background
                               // search is, admit_locked)
  j->shared = klass == 2;      // (npow_submit_sweep_shared, npow_submit_best_shared: admitted as a plain job is)
  j->count = count;
  j->pre = host_precompute(root);
  npow_asm_uniforms(j->pre.m, j->u);
  j->threshold = threshold;
  j->reserve = threshold;
  j->start = start;
  j->cancel = cancel;
  j->t_submit = now_us();
  if (count) {
    auto devs = select_gpus(device_mask);
    if (devs.empty()) return fail(NPOW_ERR_NO_DEVICE, "no usable GPU in device_mask");
    const uint64_t G = std::min<uint64_t>(devs.size(), count);
    const uint64_t per = count / G, rem = count % G;
    j->dev.resize(G);
    uint64_t off = 0;
    for (uint64_t k = 0; k < G; ++k) {
      const uint64_t part = per + (k < rem ? 1 : 0);
      j->devs.push_back(devs[k]->id);
      j->dev[k].todo.push_back({start + off, part});
      j->max_per_dev = std::max(j->max_per_dev, part);
      off += part;
    }
    j->pending_devs = (int)G;
    j->spin_us = spin_window_us(*j);
  } else {  // nothing to hash: complete at once, no device is touched
    j->status = NPOW_EXHAUSTED;
    j->decided = true;
    j->admitted = true;
    j->t_finish = j->t_submit;
    j->finished = true;
  }
  std::lock_guard<std::mutex> g(g_pool.mu);
  return enqueue_locked(j, ticket);  // (its place in the queue: a job of weight 1, foreground or background)
}

int pool_submit_sweep(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t count, uint64_t device_mask,
                      const volatile uint32_t* cancel, uint64_t* ticket, int klass) {
  return submit_collecting(root, threshold, start, count, device_mask, cancel, ticket, JobKind::kSweep, klass);
}

int pool_ticket_sweep(uint64_t ticket, npow_sweep_info* out) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP jp = ticket_job_locked(ticket);
  if (!jp) return NPOW_ERR_BAD_ARGUMENT;
  const Job& j = *jp;
  if (int rc = expect_kind(j, JobKind::kSweep, "npow_ticket_sweep", true)) return rc;
  const bool fin = j.finished.load();
  const double t = fin ? j.t_finish : now_us();
  out->background = j.background ? 1u : 0u;
  out->count = j.count;
  out->finished = fin ? 1u : 0u;
  double held = 0;
  uint64_t progress = 0;
  for (const JobDev& jd : j.dev) {
    progress += jd.progress;
    out->hits += jd.hit_n;
    out->launches += jd.launches;
    out->launches_cut += jd.launches_cut;
    held += jd.held_us + (jd.held_since > 0 && t > jd.held_since ? t - jd.held_since : 0.0);
  }
  out->nonces_done = fin ? j.done : std::max(j.done, progress);
  out->held_us = (uint64_t)held;
  return NPOW_OK;
}

int pool_wait_sweep(uint64_t ticket, int64_t timeout_us, uint64_t* out, uint64_t cap, uint64_t* n_out,
                    uint64_t* nonces_done) {
  uint64_t total = 0;
  bool lost = false;
  std::vector<uint64_t> all;
  Ended e;
  if (int rc = wait_ended(ticket, JobKind::kSweep, "npow_wait_sweep", timeout_us, &e, [&](const Job& j) {
        for (const JobDev& jd : j.dev) {
          total += jd.hit_n;
          lost = lost || jd.hits_lost || jd.hit_n > jd.hits.size();
          all.insert(all.end(), jd.hits.begin(), jd.hits.end());
        }
      }))
    return rc;
  const uint64_t start = e.job->start, count = e.job->count;
  std::sort(all.begin(), all.end(), [start](uint64_t x, uint64_t y) { return x - start < y - start; });
  const uint64_t k = std::min<uint64_t>(all.size(), cap);
  if (k) memcpy(out, all.data(), k * sizeof(uint64_t));
  *n_out = total;
  if (nonces_done) *nonces_done = e.done;
  // every nonce is hashed once, so a nonce reported twice -- or one outside the range -- is a coverage bug: never
  // deduplicated, the job fails
  for (size_t i = 0; i < all.size(); ++i)
    if (all[i] - start >= count || (i && all[i] == all[i - 1]))
      return fail(NPOW_ERR_INTERNAL, "sweep job: a hit outside the range or reported twice (nonce coverage)");
  if (e.status == NPOW_CANCELLED) return NPOW_CANCELLED;
  if (e.status < 0) return fail(e.status, e.err.empty() ? std::string("sweep job failed") : e.err);
  if (int rc = e.hashed_all("sweep job")) return rc;
  if (lost)
    return fail(NPOW_ERR_CAPACITY, "more than NPOW_SWEEP_JOB_HITS hits on a device (n_out is exact)");
  if (total > cap) return fail(NPOW_ERR_CAPACITY, "more hits than cap");
  return NPOW_OK;
}

// -- best jobs (npow_submit_best, npow_wait_best) --------------------------------------------------------------------
// The strongest nonce of [start, start + count): a sweep job's sibling (submit_collecting with kBest: the same split,
// admission and queue) whose entries keep only what beats the best so far (kEntryBest).  The workers fold each retired
// launch's records into Job::best.of (Worker::collect_best); this only reads the result.  DESIGN.md section 1 "Best
// jobs".  background (npow_submit_best_background): the class of a background sweep job -- claimed entries, held out
// while a foreground job wants the device (Job::claimed()).
int pool_submit_best(const uint8_t root[32], uint64_t floor, uint64_t start, uint64_t count, uint64_t device_mask,
                     const volatile uint32_t* cancel, uint64_t* ticket, int klass) {
  return submit_collecting(root, floor, start, count, device_mask, cancel, ticket, JobKind::kBest, klass);
}

int pool_ticket_best(uint64_t ticket, npow_best_info* out) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP jp = ticket_job_locked(ticket);
  if (!jp) return NPOW_ERR_BAD_ARGUMENT;
  const Job& j = *jp;
  if (int rc = expect_kind(j, JobKind::kBest, "npow_ticket_best")) return rc;
  const bool fin = j.finished.load();
  uint64_t progress = 0;
  for (const JobDev& jd : j.dev) {
    progress += jd.progress;
    out->launches += jd.launches;
  }
  out->count = j.count;
  out->nonces_done = fin ? j.done : std::max(j.done, progress);
  out->nonce = j.best.of.found ? j.best.of.nonce : 0;
  out->value = j.best.of.found ? j.best.of.value : 0;
  out->records = j.best.records;
  out->records_max = j.best.records_max;
  out->room = j.best.room;
  out->finished = fin ? 1u : 0u;
  return NPOW_OK;
}

// A best job's class and what it cost it (npow_ticket_best_hold), read as pool_ticket_sweep reads a sweep job's; a
// plain best job is never cut or held: zeros.
int pool_ticket_best_hold(uint64_t ticket, npow_best_hold_info* out) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP jp = ticket_job_locked(ticket);
  if (!jp) return NPOW_ERR_BAD_ARGUMENT;
  const Job& j = *jp;
  if (int rc = expect_kind(j, JobKind::kBest, "npow_ticket_best_hold")) return rc;
  const double t = j.finished.load() ? j.t_finish : now_us();
  double held = 0;
  for (const JobDev& jd : j.dev) {
    out->launches_cut += jd.launches_cut;
    held += jd.held_us + (jd.held_since > 0 && t > jd.held_since ? t - jd.held_since : 0.0);
  }
  out->background = j.background ? 1u : 0u;
  out->held_us = (uint64_t)held;
  return NPOW_OK;
}

// The class of a sweep or best job and what came with it (npow_ticket_share): plain 0, background 1, shared 2; the
// launches, the launches cut and the time held as pool_ticket_sweep and pool_ticket_best_hold report them, and the
// workgroups that moved to the job's claimed entries inside running launches (JobDev::moves).  DESIGN.md section 1
// "Shared range jobs".
int pool_ticket_share(uint64_t ticket, npow_range_share_info* out) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  const JobP jp = ticket_job_locked(ticket);
  if (!jp) return NPOW_ERR_BAD_ARGUMENT;
  const Job& j = *jp;
  if (!j.collects())
    return fail(NPOW_ERR_BAD_ARGUMENT, std::string("npow_ticket_share: the ticket is ") + kKindWords[0][0] +
                                           kKindWords[0][1]);
  const double t = j.finished.load() ? j.t_finish : now_us();
  double held = 0;
  for (const JobDev& jd : j.dev) {
    out->launches += jd.launches;
    out->launches_cut += jd.launches_cut;
    out->moves += jd.moves;
    held += jd.held_us + (jd.held_since > 0 && t > jd.held_since ? t - jd.held_since : 0.0);
  }
  out->klass = (uint32_t)j.range_class();
  out->held_us = (uint64_t)held;
  return NPOW_OK;
}

int pool_wait_best(uint64_t ticket, int64_t timeout_us, uint64_t* nonce, uint64_t* value, uint64_t* nonces_done) {
  BestFold b;
  Ended e;
  if (int rc = wait_ended(ticket, JobKind::kBest, "npow_wait_best", timeout_us, &e,
                          [&](const Job& j) { b = j.best.of; }))
    return rc;
  if (nonces_done) *nonces_done = e.done;
  if (nonce) *nonce = 0;
  if (value) *value = 0;
  if (e.status < 0) return fail(e.status, e.err.empty() ? std::string("best job failed") : e.err);
  if (int rc = e.hashed_all("best job")) return rc;
  if (b.found) {
    // (each record was recomputed when it was folded; once more, as every winner is before it is returned)
    if (host_work_value(e.job->pre.m, b.nonce) != b.value || b.nonce - e.job->start >= e.job->count)
      return fail(NPOW_ERR_INTERNAL, "best job: the best nonce failed re-validation");
    if (nonce) *nonce = b.nonce;
    if (value) *value = b.value;
  }
  if (e.status == NPOW_CANCELLED) return NPOW_CANCELLED;
  return b.found ? NPOW_OK : NPOW_EXHAUSTED;
}

int pool_set_max_active(uint32_t n) {
  if (n == 0 || n > (uint32_t)kMaxSlots)
    return fail(NPOW_ERR_BAD_ARGUMENT, "max_active must be in [1, " + std::to_string(kMaxSlots) + "]");
  std::lock_guard<std::mutex> g(g_pool.mu);
  g_pool.max_active = n;
  admit_locked();
  return NPOW_OK;
}

void pool_counts(uint32_t* queued, uint32_t* active) {
  std::lock_guard<std::mutex> g(g_pool.mu);
  if (queued) *queued = (uint32_t)g_pool.waiting.size();
  if (active) *active = (uint32_t)g_pool.active.size();
}

}  // namespace npow
