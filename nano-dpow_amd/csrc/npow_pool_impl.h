// npow_pool_impl.h -- what the work pool's own files share (npow_pool.cpp, npow_pool_jobs.cpp, npow_pool_watch.cpp;
// nothing else includes it): the environment knobs, the test hooks, the debug prints, the host's writes to a device's
// pinned mailbox, and the win watcher's interface.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "npow_pool.h"

namespace npow {

// -- environment knobs (read once; inline: one instance, a read is a plain load) ---------------------------------
inline const char* env_str(const char* name, const char* dflt) { const char* e = getenv(name); return e ? e : dflt; }
inline double env_num(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
// Between steps a worker with a launch in flight sleeps this long (wakes early on new jobs): a win is seen within it,
// and the thread costs ~6 % of a core instead of spinning (Worker::nap). NANOPOW_POLL_US overrides (0 = spin).
inline const double g_poll_us = env_num("NANOPOW_POLL_US", 50.0);
inline const bool g_debug = getenv("NANOPOW_DEBUG") != nullptr;
// Lingering launches (round 5, PoolTable::linger): an unbounded launch's workgroups wait in it for the next dynamic
// entry once its entries are over, so a serial client's next search joins the running launch instead of needing one.
// The worker ends a launch that has lingered g_linger_us with nothing to do (end_linger): its sleeping waves hold the
// CUs, and a serial client's next search comes within ~0.1 ms.  Measured on the 2^26-nonce regime, interleaved with
// the same roots (profiles/r05aj_linger_by_partition_regime_ab.jsonl): over 8 CU partitions of 32
// CUs the node rate goes 0.956 -> 0.98-0.99 of the devices' full rate with the p50 within +-0.05 ms; over 4, 2 and 1
// (64 CUs and more) it costs -- node rate 0.97-0.995 against 0.996-1.0, p50 0.04-0.19 ms later -- since each
// workgroup's acquire of a new entry (an L2 invalidation each) spreads their start, the more the more workgroups share
// an XCD.  So by default on only for CU partitions of at most kLingerMaxCus CUs (npow_pool.cpp lingers(); a
// whole GPU, and so every physical GPU of a node, launches per search); NANOPOW_LINGER=1 / 0 forces it on / off,
// NANOPOW_LINGER_US sets the wait.  Never for logical devices that time-share a GPU (Device::time_shared).
inline const int g_linger_env = getenv("NANOPOW_LINGER") ? (getenv("NANOPOW_LINGER")[0] == '0' ? 0 : 1) : -1;
inline const uint32_t g_linger_p = [] {  // NANOPOW_LINGER_P (A/B runs): the pinned-read period in looks (a power of two)
  uint32_t p = (uint32_t)atoi(env_str("NANOPOW_LINGER_P", "0")), q = 1;
  while (p && q < p) q <<= 1;
  return p ? q : 0u;
}();
inline const double g_linger_us = env_num("NANOPOW_LINGER_US", 1000.0);
// NANOPOW_READBACK=always reads every finished slot's done counts back (A/B runs; npow_pool.cpp kVerifyEvery)
inline const bool g_readback_always = strcmp(env_str("NANOPOW_READBACK", ""), "always") == 0;
// The win watcher (npow_pool_watch.cpp): on by default; NANOPOW_WATCHER=0 turns it off (A/B runs);
// NANOPOW_WATCH_NAP_US: its nap outside the spin windows (0 spins always)
inline const bool g_watcher_on = strcmp(env_str("NANOPOW_WATCHER", "1"), "0") != 0;
inline const double g_watch_nap_us = env_num("NANOPOW_WATCH_NAP_US", 20.0);
inline const bool g_trace_lat = getenv("NANOPOW_TRACE_LATENCY") != nullptr;
// NANOPOW_TRACE_STEPS=1: each pool worker times the parts of its steps (adopt, check_slots, read-back, launch, retire,
// nap) and prints count / total / max / calls over 50 us per part when it exits (diagnostics of the host path)
inline const bool g_trace_steps = getenv("NANOPOW_TRACE_STEPS") != nullptr;
// NANOPOW_WAIT_SPIN=0: result waiters sleep at once (A/B runs; npow_pool_jobs.cpp wait_job)
inline const bool g_wait_spin = env_str("NANOPOW_WAIT_SPIN", "1")[0] != '0';

// Fault injection (tests): see the header comment of npow_pool.cpp.
struct Faults {
  uint64_t invalid_mask = 0;  // logical devices whose wins read back corrupted
  int hip_dev = -1;           // logical device whose launches fail ...
  uint64_t hip_after = 0;     // ... after this many
  bool retarget_blind = false;  // pool_retarget writes no floor record
  bool no_moves = false;        // NANOPOW_SHARED_NO_MOVES: launches carry kTabNoMoves (no move to a claimed entry)
};
const Faults& faults();  // npow_pool.cpp

#define NPOW_DBG(...) \
  do { if (g_debug) fprintf(stderr, __VA_ARGS__); } while (0)
// the same with the steady clock's time first (ms; Python's time.monotonic() * 1e3 reads the same clock)
#define NPOW_DBGT(...) \
  do { if (g_debug) fprintf(stderr, "[%.3f] ", now_us() * 1e-3), fprintf(stderr, __VA_ARGS__); } while (0)

void wake_worker(Device& d);  // end its nap between two steps (npow_pool.cpp)

// -- the host's writes to a device's pinned mailbox (PoolMailbox, npow_internal.h) -----------------------------
// The waves of a running launch poll one counter word per kind of message and read a slot's own word only when the
// counter has moved.  So every message is two stores, both with release ordering: the slot's word first, then the
// counter -- a wave that sees the counter move then finds the word.  A slot's word carries the generation of the job
// in it: a slot reused later has a larger generation, so a late store could not reach another job.

// Stop the waves on slot s, generation gen: the kill word, then the low half of PoolMailbox::kills.
inline void mb_kill(Device& d, int s, uint64_t gen) {
  __atomic_store_n(&d.pmb->kill[s], gen, __ATOMIC_RELEASE);
  __atomic_fetch_add(&d.pmb->kills, 1ull, __ATOMIC_RELEASE);  // after the kill word: every poll then relays it
}
// Raise the weight of slot s, generation gen, in a running counted launch (npow_kernel.hip ls2_promo_relay): the boost
// word, then the high half of PoolMailbox::kills (promotions).
inline void mb_boost(Device& d, int s, uint64_t gen, uint32_t weight) {
  __atomic_store_n(&d.pmb->boost[s], pool_boost_word(gen, pool_wsh(weight)), __ATOMIC_RELEASE);
  __atomic_fetch_add(&d.pmb->kills, 1ull << 32, __ATOMIC_RELEASE);
}
// Move the threshold of slot s, generation gen -- a raise (pool_retarget) or a lowering (pool_relax): its floor record
// (PoolFloor), which a wave reads when it has a hit (npow_kernel.hip pool_body_ls2), so no counter.  The threshold goes
// before the generation, which is released: a wave that reads this generation then reads this threshold or a later
// one.  The same generation again (a second move): one store of the new threshold.
inline void mb_floor(Device& d, int s, uint64_t gen, uint64_t threshold) {
  PoolFloor& f = d.pmb->floor[s];
  if (__atomic_load_n(&f.gen, __ATOMIC_RELAXED) != gen) {
    __atomic_store_n(&f.threshold, threshold, __ATOMIC_RELAXED);
    __atomic_store_n(&f.gen, gen, __ATOMIC_RELEASE);
  } else {
    __atomic_store_n(&f.threshold, threshold, __ATOMIC_RELEASE);
  }
}
// A yield: the high half of PoolMailbox::ctl goes up by one (ctl: the worker's copy, only it writes the word).  Polling
// waves mark the launch's unbounded entries dead, lingering workgroups leave.
inline void mb_yield(Device& d, uint64_t& ctl) {
  ctl += 1ull << 32;
  __atomic_store_n(&d.pmb->ctl, ctl, __ATOMIC_RELEASE);
}
// The GPU slots that hold job j now (caller holds g_pool.mu): f(k, device, j.dev[k]).  Not a device that has not
// adopted it yet, nor the CPU device, which has no slot: its threads read the job's fields themselves.
template <class F>
inline void for_each_gpu_slot(Job& j, F&& f) {
  for (size_t k = 0; k < j.devs.size(); ++k) {
    JobDev& jd = j.dev[k];
    if (!jd.on || jd.slot < 0) continue;
    Device& d = *g_devs[(size_t)j.devs[k]];
    if (d.cpu_threads || !d.pmb) continue;
    f(k, d, jd);
  }
}
// Slot s's win record as the host reads it (the caller has acquired PoolWin::gen, or does so next to see whether the
// record moved on meanwhile); NANOPOW_FAULT_INVALID (tests) corrupts the value.
inline void read_win(Device& d, int s, uint64_t* nonce, uint64_t* value) {
  const PoolWin& pw = d.pmb->win[s];
  *nonce = __atomic_load_n(&pw.nonce, __ATOMIC_RELAXED);
  *value = __atomic_load_n(&pw.value, __ATOMIC_RELAXED) ^ ((faults().invalid_mask >> d.id) & 1);
}

// -- the win watcher (npow_pool_watch.cpp) ------------------------------------------------------------------------
double spin_window_us(const Job& j);  // Job::spin_us
void watch_start();                   // its thread (pool_start; nothing with NANOPOW_WATCHER=0)
void watch_stop();                    // ... stopped and joined, every slot disarmed (pool_stop, after the workers left)
void watch_arm(Device& d, int s, uint64_t gen, const JobP& j);  // the slot's win record and the job's cancel word
void watch_disarm(Device& d, int s);                            // the slot is freed
void watch_stop_cancel(Device& d, int s);                       // the slot leaves the searching state

}  // namespace npow
