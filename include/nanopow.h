/*
 * nanopow.h -- C ABI of libnanopow.so, the MI355X (gfx950) Nano proof-of-work engine.
 *
 * This library replaces the compute core of the reference's work server,
 * client/bin/windows/nano-work-server.exe (Rust + OpenCL; source not vendored,
 * upstream nanocurrency/nano-work-server v1.0).  The DPoW client never calls
 * this ABI directly: client/work_handler.py:53,75-78,104-108 talks HTTP JSON
 * to a work server, and this repository's work server
 * (nano-dpow_amd/nanopow/server.py) binds these symbols through ctypes.
 *
 * Conventions
 *   - Every function is exception-free and returns int status unless noted:
 *       NPOW_OK (0) found / done, NPOW_CANCELLED (1), NPOW_EXHAUSTED (2),
 *       negative = error; npow_last_error() then returns a thread-local message.
 *   - A root (block hash) is 32 raw bytes in the order of its hex string.
 *   - Nonces, thresholds and work values are host-endian uint64_t.  The work
 *     string a client sees is the big-endian hex of the nonce ("%016llx"),
 *     while the bytes hashed are the nonce little-endian (dpow_server.py:130).
 *   - work value = LE_u64(BLAKE2b-64(LE64(nonce) || root)); work is valid iff
 *     value >= threshold (nano-work-server.exe @1661643 `nano_work`:
 *     `if (blake2b(attempt_l, item_a) >= difficulty)`).
 *   - Buffers are caller-owned; the library keeps no pointer past a call
 *     (the `cancel` word is read only while the call runs).
 *   - A cancel word is raised from another thread with a release store
 *     (`__atomic_store_n(w, 1, __ATOMIC_RELEASE)`; an aligned 32-bit store, as
 *     ctypes makes, is one on x86-64); the library load-acquires it.
 *   - device_mask bit d selects logical device d (HIP device d, or d mod the HIP
 *     devices under NANOPOW_VIRTUAL_DEVICES, a test setting); 0 means "all devices".
 *   - Calls that use disjoint device sets may run concurrently from
 *     different threads; calls that share a device serialise on it.
 */
#ifndef NANOPOW_H
#define NANOPOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPOW_OK 0
#define NPOW_CANCELLED 1
#define NPOW_EXHAUSTED 2
#define NPOW_PENDING 3             /* npow_wait: timeout elapsed, the ticket is still valid */
#define NPOW_TOO_LATE 4   /* npow_retarget, npow_relax: the search was already decided or cancelled (not yet collected); unchanged */
#define NPOW_ERR_NOT_INITIALISED (-1)
#define NPOW_ERR_NO_DEVICE (-2)
#define NPOW_ERR_BAD_ARGUMENT (-3)
#define NPOW_ERR_HIP (-4)
#define NPOW_ERR_INVALID_WORK (-5) /* a job's last device was dropped for 3 invalid results in a row */
#define NPOW_ERR_CAPACITY (-6)     /* sweep found more hits than `cap` (n_out still exact) */
#define NPOW_ERR_INTERNAL (-7)     /* host-side failure (out of memory, thread creation); no C++
                                      exception ever crosses this ABI */

/* ABI revision (npow_abi_version()).  3: npow_values runs the search kernels' stream;
 * npow_values_path, npow_wait_info, npow_device_stats_get_sized added;
 * npow_device_stats_get writes only the revision-2 prefix of npow_device_stats.
 * 4: npow_config_cpu_threads (CPU workers, --cpu-threads), npow_wait_result (the outcome at the decision);
 * npow_device_stats gains late_nonces,
 * hip_device, cu_first; npow_search_info gains late_nonces_losers / late_nonces_winner (both structs
 * are written up to the size the caller passes, so revision-3 callers are unaffected).
 * 5: npow_search_info gains the search's host timeline (adopt_us, launch_us, launch_all_us, win_seen_us);
 * npow_device_stats gains idle_ms / idle_gaps (the GPU idle between the device's search launches) and
 * affinity_checks / affinity_failures (NANOPOW_TEST_HOOKS=1, since npow_init: the calling thread's HIP device checked
 * at every HIP call site of the device) and watcher_decisions.  Both structs are still written up to the size the caller passes.
 * 6: npow_device_stats gains stale_drains / stale_late / stale_missing / stale_gpu_delay_us (won or killed jobs of a
 * lingering launch whose final count had not come 1 ms after their stop; of those, the ones whose count came later and
 * the ones whose count never came -- a protocol check: 0), linger_ms (the device's lingering launches waiting with
 * nothing to hash, inside kernel_ms) and linger_relays (kills relayed by a lingering workgroup).
 * 7: npow_submit_weighted (a job's weight: its share of each GPU among the live searches, and its place in the
 * admission queue); npow_submit is the same call with weight 1.
 * Added within revision 7 (the number stays; callers probe for the symbol): npow_promote (raise the weight of a
 * search that is waiting or running), and npow_device_stats gains promotions (still written up to the caller's size);
 * npow_retarget (raise the threshold of a search that is waiting or running; NPOW_TOO_LATE), and npow_search_info
 * gains retargets / stale_hits / stale_wins (likewise written up to the caller's size); npow_submit_background (a
 * search that hashes only on workgroups no other search wants) and npow_ticket_background (its class now);
 * npow_submit_reserve (a search that keeps the best nonce it passes between a reserve threshold and its own),
 * npow_ticket_reserve (a look at that nonce) and npow_relax (lower the threshold of a running search, answered at once
 * from the reserve when it qualifies), with NPOW_RESERVE_MIN and npow_reserve_info; the sweep jobs
 * (npow_submit_sweep, npow_wait_sweep, npow_submit_sweep_background, npow_ticket_sweep) and the best jobs
 * (npow_submit_best, npow_wait_best, npow_ticket_best, npow_submit_best_background, npow_ticket_best_hold: the
 * strongest nonce of a range), each described at its
 * declaration. */
#define NPOW_ABI_VERSION 7

/* The lowest reserve threshold npow_submit_reserve takes.  A wave of a search with a reserve enters the kernel's rare
 * branch whenever one of its 64 lanes meets the reserve: once in 2^14 hashes here (0.06 % even if the branch cost ten
 * hash times); below it the branch stops being rare.  The receive difficulty, fffffe0000000000, is well inside. */
#define NPOW_RESERVE_MIN 0xfffff00000000000ull

/* Hash paths of npow_values_path. */
#define NPOW_PATH_SEARCH 0  /* the instruction stream the search and sweep kernels execute
                               (npow_hash_asm_lockstep_ld.inc, four 512-lane workgroups per CU) */
#define NPOW_PATH_SEQ 1     /* a second generated stream, scheduled without barriers (npow_hash_asm.inc) */
#define NPOW_PATH_GENERIC 2 /* plain HIP C++ of the 12 rounds, one (root, nonce) per lane */

/* Per-device counters; kernel_ms is measured with HIP events recorded on the
 * stream each kernel is launched on (bench.py's roofline leg reads these). */
typedef struct npow_device_stats {
  uint64_t launches;      /* kernel launches (search + sweep + values) */
  uint64_t nonces;        /* nonces whose hash the kernels computed */
  double kernel_ms;       /* sum of per-launch event-timed durations */
  uint64_t invalid_work;  /* GPU winners rejected by CPU re-validation */
  int32_t cus;            /* compute units */
  int32_t grid;           /* workgroups per search/sweep launch */
  double clock_mhz;       /* in-kernel shader clock of the search launches since the last reset:
                             s_memtime / s_memrealtime spans of one wave per XCD (0 = none yet) */
  double host_cpu_ms;     /* CPU time of the device's pool worker thread since the last reset */
  double host_wall_ms;    /* wall time since the last reset (host_cpu_ms / host_wall_ms = the
                             worker's share of one core) */
  int32_t dead;           /* 1 once the device has been dropped: 3 invalid results in a row
                             (nano-work-server.exe @1669144) or a failed HIP call; searches then
                             skip it and its jobs' remaining ranges move to the other devices */
  int32_t pool_groups;    /* workgroups per CU of the search kernel (npow_pool_kernel_ls2*): 4
                             512-lane ones -- 8 waves per SIMD either way; earlier ABI-3 libraries
                             ran 2 of 1,024 lanes, revisions before ABI 3 also had 0 = seq, 1 */
  uint64_t early_finishes;  /* jobs finished from the kernel's published final count (search
                               kernels): a won or killed entry's count once no workgroup is left on
                               it, before the launch that held it ends */
  uint64_t early_mismatches; /* of those, counts that the read-back after the launch contradicted
                               (always 0: a protocol check) */
  uint64_t yields;          /* running launches ended early so that new jobs could start */
  uint64_t dyn_entries;     /* jobs that joined a running launch instead (no yield) */
  /* ---- ABI 3 (npow_device_stats_get_sized only) ---- */
  uint64_t kills_relayed;   /* losing jobs of this device stopped by another device's win: the deciding
                               thread raised this device's kill word directly (no wait for its worker) */
  /* ---- ABI 4 ---- */
  uint64_t late_nonces;     /* device-side overshoot of the search kernels: nonces hashed by workgroups in
                               iterations that started after one of their waves knew the job was over (its
                               dead word, a win, a kill read by a poll) -- counted in the kernel */
  int32_t hip_device;       /* HIP device this logical device runs on (-1: the CPU workers) */
  int32_t cu_first;         /* -1: the whole GPU; else the first CU of its partition (NANOPOW_VIRTUAL_DEVICES:
                               a CU-masked stream over CUs [cu_first, cu_first + cus)) */
  /* ---- ABI 5 ---- */
  double idle_ms;           /* GPU idle on the device's stream between consecutive search launches: from one
                               launch's stop event to the next one's start event (HIP events), summed */
  uint64_t idle_gaps;       /* ... over this many pairs of consecutive launches */
  uint64_t affinity_checks; /* NANOPOW_TEST_HOOKS=1: HIP call sites of this device at which the calling thread's
                               current HIP device was checked (hipGetDevice == hip_device) ... */
  uint64_t affinity_failures; /* ... and found wrong (the call then fails: NPOW_ERR_INTERNAL) */
  uint64_t watcher_decisions; /* jobs decided by the process's win watcher from this device's win records (it spins
                                 over every live slot's record; NANOPOW_WATCHER=0 leaves them to the device's worker) */
  /* ---- ABI 6 ---- */
  uint64_t stale_drains;    /* won or killed jobs of a lingering launch whose final count the kernel had not published
                               1 ms after the stop (the worker then ended the launch and read the count back) */
  double linger_ms;         /* of kernel_ms, the time this device's lingering launches waited with nothing to hash
                               (host-timed): (kernel_ms - linger_ms) is the time the device hashed */
  uint64_t linger_relays;   /* final counts published after a lingering workgroup relayed the kill of an entry that
                               no workgroup was hashing (ls2_linger_relay; without it the count never came) */
  uint64_t stale_late;      /* of stale_drains: the count was published later after all (the GPU was late) ... */
  uint64_t stale_missing;   /* ... or never, though every launch that held the job ended: a protocol hole, 0 */
  double stale_gpu_delay_us; /* the latest such late count's publish after the job's deciding win, on the GPU's clock
                                (s_memrealtime; one clock over CU partitions of one GPU, not across GPUs) */
  /* ---- ABI 7, with npow_promote ---- */
  uint64_t promotions;      /* promotions (npow_promote) this device published into a running launch: the launch
                               rebalanced its workgroups to the new weight without ending */
} npow_device_stats;

/* Outcome of one search (npow_wait_info).  Times are host steady-clock microseconds since
 * npow_submit.  For a job split over several devices, the other devices keep hashing from the
 * moment the host accepts the winner until their waves have left the job: stop_after_decide_us is
 * the longest such span among them as the host observed it (the device's worker saw the job's
 * final count or the launch that held it complete -- so an upper bound of the device time), and
 * overshoot_nonces the sum over them of that span times the device's kernel rate (likewise an
 * upper bound of the nonces hashed after the decision).  Both are 0 for a one-device job. */
typedef struct npow_search_info {
  uint32_t size;            /* set by the caller: sizeof(npow_search_info) it was compiled with */
  int32_t status;           /* as npow_wait returns it */
  uint64_t nonce, value;    /* valid when status == NPOW_OK */
  uint64_t nonces_done;     /* every device, including the rest of a launch after the win */
  int32_t winner_device;    /* logical device whose result decided the job; -1 if none */
  int32_t n_devices;        /* devices the job was split over */
  double decide_us;         /* the winner accepted (CPU re-validated) */
  double finish_us;         /* every device done with the job */
  double stop_after_decide_us;
  uint64_t overshoot_nonces;
  /* ---- ABI 4: counted on the devices (npow_device_stats.late_nonces, per job) ---- */
  uint64_t late_nonces_losers;  /* nonces the other devices' waves hashed for the job after they knew it was
                                   over (the kill relayed into their dead word); the host-side bound above
                                   adds the kill's way there and the worker's observation */
  uint64_t late_nonces_winner;  /* the same on the deciding device after its own win */
  /* ---- ABI 5: the search's host timeline (us since npow_submit; 0 = it did not happen) ---- */
  double adopt_us;          /* the first device's pool worker took the job */
  double launch_us;         /* the first launch holding it was issued (any device) */
  double launch_all_us;     /* every device of the job had issued a launch holding it */
  double win_seen_us;       /* the deciding device's winner record was read by the host (decide_us follows its CPU
                               re-validation) */
  /* ---- ABI 7, with npow_retarget ---- */
  uint64_t retargets;       /* raises of the search's threshold that took effect */
  uint64_t stale_hits;      /* lanes whose value met an older threshold but not the current one, refused on the GPU:
                               the search went on in place */
  uint64_t stale_wins;      /* wins a device published under an older threshold: the host refused them and re-armed
                               the search on that device (the fallback; not invalid work) */
} npow_search_info;

/* CPU workers (nano-work-server.exe @1681064 `--cpu-threads N`): before npow_init, ask it to add
 * `threads` host threads (0 = none, the default; at most 1024) as one more logical device after the
 * GPUs.  Searches whose device_mask selects it (mask 0 = all devices does) give it a stride of
 * their own like a GPU; its threads hash with the library's own CPU work value (the function that
 * re-validates GPU winners), one job at a time, and the first valid result from any device decides
 * the job.  Sweeps and values run on GPUs only.  npow_init still fails without a GPU: the CPU workers
 * run beside GPUs, never instead of them.  Its npow_device_stats has hip_device = -1, cus = threads.
 * NPOW_ERR_BAD_ARGUMENT after npow_init. */
int npow_config_cpu_threads(uint32_t threads);

/* Open every visible HIP device, create its stream and buffers.
 * Replaces the work server's OpenCL device set-up for `--gpu P:D[:THREADS]`
 * (nano-work-server.exe @1681064).  Idempotent. */
int npow_init(int* n_devices);

/* Release every device resource.  Safe to call more than once. */
void npow_shutdown(void);

/* Thread-local description of the last error on this thread ("" if none). */
const char* npow_last_error(void);

/* CPU work value of one (root, nonce): the CPU re-validation the work server
 * applies to every GPU result ("GPU returned invalid work", nano-work-server.exe
 * @1669040) and the `work_validate` action (@1680400..1680528). */
uint64_t npow_work_value(const uint8_t root[32], uint64_t nonce);

/* First-win search: scan the nonce space from `start` on every device in
 * `device_mask` (device k of G starts at start + k*2^64/G, disjoint strides) until one
 * value >= threshold is found (NPOW_OK), `*cancel` becomes non-zero
 * (NPOW_CANCELLED), or every device's range [start_k, start_k + max_nonces_per_device)
 * (0 = unbounded) has been hashed without a hit (NPOW_EXHAUSTED).
 * Replaces the kernel `nano_work` (nano-work-server.exe @1661643) and the work
 * server's GPU loop behind `work_generate` (@1673856 reply fields work /
 * difficulty / multiplier, "Cancelled" @1673856).  Every GPU winner is
 * re-validated on the CPU before it is returned.
 * The search is a job of the engine's work pool (= npow_submit + npow_wait): it runs
 * in the same kernel launches as every other job in flight on those devices.
 * `cancel` may be NULL.  `nonces_done` (may be NULL) receives the number of
 * nonces hashed by all devices, including the rest of a chunk after the win. */
int npow_search(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t device_mask,
                uint64_t max_nonces_per_device, const volatile uint32_t* cancel,
                uint64_t* nonce_out, uint64_t* value_out, uint64_t* nonces_done);

/* Batched first-win search over n roots (the DPoW burst: many work_generate
 * requests in flight at once, client/work_handler.py:83-125 per client).
 * Each root i gets its own threshold and its own cancel word cancel[i]
 * (cancel itself or any entry may be NULL) and is searched by every device in
 * device_mask; up to the pool's max_active roots share each kernel launch.
 * status_out[i] is NPOW_OK / NPOW_CANCELLED / NPOW_EXHAUSTED (or an error) per
 * root; *nonces_done = nonces hashed for all roots.  Returns NPOW_OK or the
 * first negative error. */
int npow_search_batch(const uint8_t* roots, const uint64_t* thresholds, uint32_t n,
                      uint64_t device_mask, uint64_t max_nonces_per_root,
                      const volatile uint32_t* const* cancel, uint64_t* nonces_out,
                      uint64_t* values_out, int32_t* status_out, uint64_t* nonces_done);

/* ---- Work pool: asynchronous first-win searches ----------------------------------
 * Every search is a job of the engine's pool.  Jobs queue FIFO; up to max_active
 * (default and maximum 64) are live at once, and each device searches all of its
 * live jobs in ONE kernel launch (a job won or cancelled mid-launch hands its waves
 * to the others).  Replaces the work server's request queue (nano-work-server.exe
 * @1679680 `status` generating / queue_size) with concurrent service.
 *
 * npow_submit: queue a search (arguments as npow_search) and return at once with a
 * ticket.  `cancel` (may be NULL) must stay valid until npow_wait returns a final
 * status for the ticket. */
int npow_submit(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t device_mask,
                uint64_t max_nonces_per_device, const volatile uint32_t* cancel, uint64_t* ticket);

/* npow_submit with a weight in {1, 2, 4, 8} (ABI 7); npow_submit is weight 1.  Among the live unbounded searches of
 * one GPU a job's expected share of the device's workgroups -- and so of its hash rate -- is weight / (sum of the
 * weights): an on-demand request of weight 8 among 15 precache requests of weight 1 gets 8/23 of the GPU instead of
 * 1/16.  A job split over several devices carries its weight on each of them; the CPU workers (one job at a time)
 * ignore it.  Waiting jobs (more than max_active submitted) are admitted heaviest first, first come first served
 * within a weight.  NPOW_ERR_BAD_ARGUMENT for any other weight, and for a weight above 1 together with
 * max_nonces_per_device != 0 (a bounded search is covered by its own workgroups only). */
int npow_submit_weighted(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t device_mask,
                         uint64_t max_nonces_per_device, const volatile uint32_t* cancel, uint32_t weight,
                         uint64_t* ticket);

/* Queue a background search (added within ABI 7; probe for the symbol): an unbounded search, as npow_submit with
 * max_nonces_per_device = 0, that each GPU hashes only on the workgroups no foreground search -- every search queued
 * by the other calls -- wants.  This is a class, not a small weight: while a foreground search is live in a device's
 * launch, the launch's background searches hold no workgroup there (they keep their slots and nonce positions), and
 * they get the workgroups back as soon as the foreground searches end -- inside the running launch, nothing ends or
 * restarts.  Background searches alone share a device equally.  npow_promote(ticket, w) makes the search foreground
 * with weight w, whether it is waiting, admitted or inside a running launch; npow_retarget and npow_cancel work as on
 * any search (npow_ticket_background tells how it ended).  Admission: waiting background searches are admitted
 * after every waiting foreground one, first come first served, only while fewer than max_active searches are live, and
 * never to more than half of the 64 slots; a foreground search is admitted while fewer than max_active foreground
 * searches are live and a slot is free, so it never waits behind background ones.  In a launch that holds a bounded
 * search the device's background searches run as foreground searches of weight 1 for that launch.  The CPU workers
 * ignore the class. */
int npow_submit_background(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t device_mask,
                           const volatile uint32_t* cancel, uint64_t* ticket);

/* The class of an uncollected ticket's search (added within ABI 7; probe for the symbol): *background = 1 while it is
 * a background search, 0 for a foreground one and once npow_promote has lifted it.  A decided search's class no longer
 * changes, so read after npow_wait_result and before npow_wait / npow_wait_info it is the class the search ended in.
 * (npow_search_info keeps its revision-7 layout, which ends with stale_wins.)  NPOW_ERR_BAD_ARGUMENT for an unknown or
 * collected ticket. */
int npow_ticket_background(uint64_t ticket, uint32_t* background);

/* Wait up to timeout_us (< 0: forever) for a ticket.  Returns NPOW_PENDING on timeout
 * (the ticket stays valid), otherwise the search's final status exactly as npow_search
 * returns it; the ticket is released then.  Outputs as npow_search. */
int npow_wait(uint64_t ticket, int64_t timeout_us, uint64_t* nonce_out, uint64_t* value_out,
              uint64_t* nonces_done);

/* npow_wait with the search's outcome and timeline in *info (info->size set by the caller; the
 * library writes at most that many bytes).  Returns as npow_wait. */
int npow_wait_info(uint64_t ticket, int64_t timeout_us, npow_search_info* info);

/* The search's outcome as soon as it is known (ABI 4): NPOW_OK with nonce / value once a winner has passed
 * CPU re-validation, NPOW_CANCELLED once the cancellation is seen, NPOW_EXHAUSTED or an error when the search
 * ends so, NPOW_PENDING on timeout.  Unlike npow_wait it does not wait for the other devices of a split
 * search to stop, nor release the ticket: collect it with npow_wait / npow_wait_info afterwards (nonces_done
 * is complete only there), and keep the cancel word valid until then.  The reference work server answers a
 * work_generate as soon as its result validates (nano-work-server.exe @1669040); the JSON server here replies
 * at this point and collects the ticket after the reply. */
int npow_wait_result(uint64_t ticket, int64_t timeout_us, uint64_t* nonce_out, uint64_t* value_out);

/* Cancel a ticket (same effect as raising its cancel word). */
int npow_cancel(uint64_t ticket);

/* Raise the weight of a search that is waiting, admitted or running (added within ABI 7; probe for the symbol):
 * the job's weight becomes max(current, weight), weight in {1, 2, 4, 8}.  A waiting job moves up the admission queue
 * (heaviest first, first come first served within a weight).  A job inside a running launch of several searches gets
 * its new share within that launch -- the launch's workgroups rebalance, nothing ends or restarts (npow_device_stats
 * promotions counts these) -- and every later launch carries the weight; on each device of a split job, the CPU
 * workers ignoring it.  NPOW_OK and no change for a weight at or below the current one, and for a search already
 * decided or cancelled but not yet collected.  NPOW_ERR_BAD_ARGUMENT for any other weight, an unknown or collected
 * ticket, and a weight above 1 on a bounded search.  Never waits for a GPU.  A weight is never lowered.
 * A background search (npow_submit_background) becomes a foreground search of weight `weight` -- any of 1, 2, 4, 8 --
 * in every one of those states; inside a running launch its workgroups arrive through the same rebalancing. */
int npow_promote(uint64_t ticket, uint32_t weight);

/* Raise the threshold of a search that is waiting, admitted or running (added within ABI 7; probe for the symbol):
 * the job's threshold becomes max(current, threshold) -- this call never lowers it (npow_relax does, for a search
 * with a reserve), and a threshold at or below the current one is NPOW_OK with no effect.  Nothing ends or restarts: the search keeps its slot, its weight and its place in the
 * nonce space on every device of a split job, the GPUs pass over hits that no longer qualify (npow_search_info
 * stale_hits) and the CPU workers compare with the current threshold.  A search with a reserve (npow_submit_reserve)
 * passes over them too: until the running launch ends, the hits between the old threshold and the new one do not
 * reach its reserve.  After NPOW_OK every result the ticket returns
 * has value >= threshold.  NPOW_TOO_LATE when the search was already decided, cancelled or finished (not yet
 * collected): its result stands and may be below `threshold`.  NPOW_ERR_BAD_ARGUMENT for an unknown or collected
 * ticket.  Bounded searches are accepted: the threshold does not touch their coverage.  Never waits for a GPU. */
int npow_retarget(uint64_t ticket, uint64_t threshold);

/* Queue a search with a reserve threshold (added within ABI 7; probe for the symbol): an unbounded search, as
 * npow_submit_weighted with max_nonces_per_device = 0 -- a background one with background != 0, as
 * npow_submit_background (its weight then only checked) -- that also remembers, on each GPU, the best nonce it has
 * passed whose value is in [reserve, threshold): its reserve.  `threshold` is the current one, with one exception:
 * in the launch that is running when npow_retarget raises the search, the values between the threshold that
 * launch's entry was built with and the raised one are counted as stale hits and are NOT kept (a later npow_relax to
 * a level among them is lowered in place, not answered at once); every later launch keeps them.  The hot loop is
 * the same (it compares with `reserve`
 * and sorts the rare hits afterwards), so the reserve costs nothing per nonce.  npow_ticket_reserve looks at it,
 * npow_relax lowers the search's threshold to any level down to `reserve`.  reserve == threshold is npow_submit_weighted
 * / npow_submit_background itself.  NPOW_ERR_BAD_ARGUMENT for reserve > threshold, reserve < NPOW_RESERVE_MIN and a
 * weight other than 1, 2, 4, 8.  The CPU workers compare with the current threshold and keep no reserve. */
int npow_submit_reserve(const uint8_t root[32], uint64_t threshold, uint64_t reserve, uint64_t start,
                        uint64_t device_mask, const volatile uint32_t* cancel, uint32_t weight, uint32_t background,
                        uint64_t* ticket);

/* A search's reserve (npow_ticket_reserve).  A struct of its own: npow_search_info keeps ending with stale_wins and
 * npow_device_stats with promotions. */
typedef struct npow_reserve_info {
  uint32_t size;        /* set by the caller; the library writes at most that many bytes */
  uint32_t armed;       /* 1: submitted with reserve < threshold */
  uint64_t reserve_threshold, threshold;   /* threshold: the current one */
  uint64_t nonce, value;  /* best reserve held, CPU-validated; value 0 = none yet */
  int32_t device;       /* logical device that found it; -1 = none */
  uint32_t answered;    /* 1: npow_relax decided the search from its reserve */
  uint64_t relaxes;     /* lowerings that took effect */
  uint64_t candidates;  /* reserve records read from the GPUs and validated */
} npow_reserve_info;

/* Look at the reserve of an uncollected ticket's search without disturbing it (added within ABI 7; probe for the
 * symbol): reads the reserve record of every GPU that holds the search, validates each new nonce on the CPU
 * (npow_work_value) and keeps the best.  A GPU's record is a hint -- only its nonce is used, so a torn or stale
 * record recomputes to a low value and is dropped; it is never invalid work.  NPOW_OK with out->value == 0 while
 * there is none.  NPOW_ERR_BAD_ARGUMENT for an unknown or collected ticket, or out / out->size missing.  Never
 * waits for a GPU. */
int npow_ticket_reserve(uint64_t ticket, npow_reserve_info* out);

/* Lower the threshold of a search submitted with a reserve (added within ABI 7; probe for the symbol): the
 * threshold becomes min(current, threshold); *answered (may be null) tells how.  The reserves are harvested as by
 * npow_ticket_reserve; if the best one has value >= threshold the search is decided from it at once (*answered = 1)
 * -- its result is available to npow_wait_result before this returns, every device's waves are told to stop and the
 * final counts arrive as after any win: no GPU wait, no launch.  Otherwise the lowered threshold is published to every
 * device's running launch and carried by every later one (*answered = 0; a reserve that arrived meanwhile still
 * answers), and the next lane at or above it wins; nothing ends or restarts.  After NPOW_OK every result the ticket
 * returns has value >= the lowered threshold.  NPOW_OK with no effect for a threshold at or above the current one.
 * NPOW_TOO_LATE when the search was already decided or cancelled.  NPOW_ERR_BAD_ARGUMENT for a threshold below the
 * search's reserve threshold, a search without a reserve, and an unknown or collected ticket.  Composes with
 * npow_retarget: the current threshold moves both ways and is never below the reserve threshold.  Never waits for a
 * GPU. */
int npow_relax(uint64_t ticket, uint64_t threshold, uint32_t* answered);

/* Jobs searched at once (1..64).  Fewer gives the oldest requests every GPU sooner
 * (lower time-to-work under load); more keeps waves busy when jobs end mid-launch. */
int npow_pool_config(uint32_t max_active);

/* Jobs queued (not yet live) and live. */
int npow_pool_status(uint32_t* queued, uint32_t* active);

/* Exhaustive sweep: every nonce in [start, start+count) (mod 2^64) whose value
 * >= threshold, written to out[0..min(n,cap)) in ascending (nonce - start)
 * order; *n_out = exact hit count.  The range is split into contiguous parts
 * over the devices in device_mask.  Returns NPOW_ERR_CAPACITY when n > cap
 * (out then holds the first cap hits), NPOW_CANCELLED if *cancel fired. */
int npow_sweep(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t count,
               uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* out, uint64_t cap,
               uint64_t* n_out);

/* Sweep jobs (added within ABI 7; probe for the symbols): the same enumeration as a job of the work pool.  npow_sweep
 * takes each device from the pool for as long as it runs -- every search on it waits -- whereas a sweep job has a
 * ticket and shares the pool's launches with up to 63 other jobs: it is hashed by the kernels that answer searches,
 * a bounded job whose hits are collected instead of ending it.
 *
 * npow_submit_sweep returns at once.  Any threshold; [start, start + count) is taken mod 2^64 and split into contiguous
 * parts over the GPUs of device_mask (0 = all), as npow_sweep splits it; the CPU workers take no part.  The job takes a
 * slot like a bounded search (weight 1, foreground), counts against npow_pool_config's limit and queues like any job.
 * count == 0 completes at once with no hits and touches no device.
 *
 * npow_wait_sweep alone collects such a ticket.  NPOW_PENDING when timeout_us (< 0: none) passes first; the ticket
 * stays valid.  NPOW_OK: every nonce of the range was hashed exactly once; out[0..min(n, cap)) holds the hits in
 * ascending (nonce - start) order, *n_out = n, the exact hit count, *nonces_done (may be null) = count.
 * NPOW_ERR_CAPACITY: more hits than cap, or more than NPOW_SWEEP_JOB_HITS on one device; *n_out is still exact and
 * out holds the first hits.  NPOW_CANCELLED after npow_cancel or *cancel: out holds the hits found so far, ascending,
 * *n_out their number, *nonces_done what was hashed.  A device dropped while it holds the job fails the job with that
 * device's error: a part of the range is never hashed again elsewhere, which would report hits twice.  A hit reported
 * twice is NPOW_ERR_INTERNAL, never deduplicated.  Every status but NPOW_PENDING releases the ticket.
 *
 * npow_cancel works on a sweep job's ticket.  npow_promote, npow_retarget, npow_relax, npow_ticket_reserve,
 * npow_ticket_background, npow_wait, npow_wait_info and npow_wait_result return NPOW_ERR_BAD_ARGUMENT and leave it
 * collectable, as npow_wait_sweep does for a search's ticket. */
#define NPOW_SWEEP_JOB_HITS 1048576 /* hits one device keeps for one sweep job (2^20, npow_sweep's device buffer) */
int npow_submit_sweep(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t count,
                      uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket);
int npow_wait_sweep(uint64_t ticket, int64_t timeout_us, uint64_t* out, uint64_t cap, uint64_t* n_out,
                    uint64_t* nonces_done);

/* Background sweep jobs (added within ABI 7; probe for the symbols): a sweep job that each GPU hashes only while no
 * foreground job wants that GPU -- the class npow_submit_background gives a search, for the enumeration.  Same
 * arguments and same split of the range as npow_submit_sweep; npow_wait_sweep collects the ticket with the same
 * statuses and guarantees (NPOW_OK: every nonce hashed exactly once, hits strictly ascending by nonce - start, *n_out
 * exact past the capacity, a duplicate is NPOW_ERR_INTERNAL, a dropped device fails the job); npow_cancel works on
 * it; every other ticket call refuses it as it refuses any sweep ticket, npow_promote included (a background sweep job
 * cannot be lifted to a foreground one).  count == 0 completes at once.
 *
 * On each device the job's part is hashed only in launches built while no foreground job is live on that device or
 * waiting for it: searches from every other submit call, bounded searches and plain sweep jobs are foreground;
 * background searches are not, and share a launch with the job as they do with a bounded search.  While held out the
 * job keeps its slot, its generation and its place in the range.  A launch that holds it takes its span in chunks of
 * 8,192 nonces per workgroup and ends within one chunk (~0.3 ms) once a foreground job arrives or the launch's time
 * budget (npow_set_pool_tuning) passes; what it did not reach goes back to the job.  It is admitted as background
 * searches are: behind every waiting foreground job, under the same cap on slots.
 * CONTINUOUS FOREGROUND LOAD STARVES IT: the job makes no progress while any foreground job is live on its devices,
 * for as long as that lasts.  That is the meaning of the class. */
int npow_submit_sweep_background(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t count,
                                 uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket);

/* A look at an uncollected sweep ticket, plain or background (npow_ticket_sweep). */
typedef struct npow_sweep_info {
  uint32_t size;          /* set by the caller; the library writes at most that many bytes */
  uint32_t background;    /* 1: npow_submit_sweep_background */
  uint64_t count;         /* nonces of the job's range */
  uint64_t nonces_done;   /* nonces credited by the launches retired so far (the final count once finished) */
  uint64_t hits;          /* hits read from the launches retired so far */
  uint64_t launches;      /* launches that held an entry of the job, summed over its devices */
  uint64_t launches_cut;  /* of those, launches that ended with part of their span unhashed: a yield or the time
                           * budget (background jobs only; the part went back to the job) */
  uint64_t held_us;       /* time the job sat admitted but left out of its devices' tables, summed over its devices */
  uint32_t finished;      /* 1: npow_wait_sweep would return at once */
  uint32_t pad;
} npow_sweep_info;

/* Progress of an uncollected sweep job's ticket (added within ABI 7; probe for the symbol).  Written up to out->size.
 * NPOW_ERR_BAD_ARGUMENT for a search's ticket, an unknown or collected one, or out / out->size missing.  Never waits
 * for a GPU. */
int npow_ticket_sweep(uint64_t ticket, npow_sweep_info* out);

/* Best jobs (added within ABI 7; probe for the symbols): the nonce of [start, start + count) with the highest work
 * value, as a job of the work pool -- "hash exactly count nonces for this root and give me the strongest".  A sweep
 * job's sibling: hashed by the kernels that answer searches, in launches shared with up to 63 other jobs, but its
 * waves compare with the best value seen so far instead of a fixed threshold and record only what beats it, so the
 * answer is exact at any floor (0 included) and costs no instruction per nonce.
 *
 * npow_submit_best returns at once.  Only nonces with value >= floor are candidates; any floor, 0 allowed.  The range
 * is taken mod 2^64 and split into contiguous parts over the GPUs of device_mask (0 = all) exactly as
 * npow_submit_sweep splits it; the CPU workers take no part.  The job is a foreground job of weight 1: it takes a
 * slot, counts against npow_pool_config's limit and queues like a bounded search.  count == 0 completes at once
 * (NPOW_EXHAUSTED) and touches no device.
 *
 * npow_wait_best alone collects such a ticket.  NPOW_PENDING when timeout_us (< 0: none) passes first; the ticket
 * stays valid.  NPOW_OK: every nonce of the range was hashed exactly once, *value_out is the maximum work value of
 * the range, *nonce_out the nonce that has it -- among nonces of equal value the one with the smallest nonce - start
 * -- and *nonces_done (may be null) == count.  NPOW_EXHAUSTED: the range was hashed in full and no value reached
 * floor; *nonces_done == count.  NPOW_CANCELLED after npow_cancel or *cancel: the best candidate found so far, if
 * any (*value_out == 0: none), and *nonces_done what was hashed.  The nonce is re-validated on the CPU
 * (npow_work_value) before it is returned.  A device dropped while it holds the job fails the job with that device's
 * error, and a launch that recorded more candidates than its records hold (at least 16,384; tens are expected) fails
 * it with NPOW_ERR_INTERNAL rather than return a possibly wrong answer.  Every status but NPOW_PENDING releases the
 * ticket.
 *
 * npow_cancel works on a best job's ticket.  npow_wait, npow_wait_info, npow_wait_result, npow_wait_sweep,
 * npow_ticket_sweep, npow_promote, npow_retarget, npow_relax, npow_ticket_reserve and npow_ticket_background return
 * NPOW_ERR_BAD_ARGUMENT and leave it collectable, as npow_wait_best and npow_ticket_best do for every other kind of
 * ticket. */
int npow_submit_best(const uint8_t root[32], uint64_t floor, uint64_t start, uint64_t count,
                     uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket);
int npow_wait_best(uint64_t ticket, int64_t timeout_us, uint64_t* nonce_out, uint64_t* value_out,
                   uint64_t* nonces_done);

/* A look at an uncollected best ticket (npow_ticket_best). */
typedef struct npow_best_info {
  uint32_t size;          /* set by the caller; the library writes at most that many bytes */
  uint32_t finished;      /* 1: npow_wait_best would return at once */
  uint64_t count;         /* nonces of the job's range */
  uint64_t nonces_done;   /* nonces credited by the launches retired so far (the final count once finished) */
  uint64_t nonce, value;  /* the best candidate of the launches retired so far (value 0: none yet) */
  uint64_t launches;      /* launches that held an entry of the job, summed over its devices */
  uint64_t records;       /* candidates those launches recorded, all told ... */
  uint64_t records_max;   /* ... and the most one launch's entry recorded */
  uint64_t room;          /* the fewest records one of its entries had room for (0: no launch retired yet) */
} npow_best_info;

/* Progress of an uncollected best job's ticket (added within ABI 7; probe for the symbol).  Written up to out->size.
 * NPOW_ERR_BAD_ARGUMENT for any other kind of ticket, an unknown or collected one, or out / out->size missing.  Never
 * waits for a GPU. */
int npow_ticket_best(uint64_t ticket, npow_best_info* out);

/* Background best jobs (added within ABI 7; probe for the symbols): a best job that each GPU hashes only while no
 * foreground job wants that GPU -- the class npow_submit_sweep_background gives a sweep job, for the strongest nonce:
 * strengthen the work held for a root with whatever the GPUs have left, and look at the best so far at any time
 * (npow_ticket_best).  Same arguments and same split of the range as npow_submit_best; npow_wait_best,
 * npow_ticket_best and npow_cancel work on the ticket exactly as on a plain best job's, with the same statuses and
 * guarantees (NPOW_OK: every nonce hashed exactly once, the maximum of the range, the smallest nonce - start among
 * equal values, *nonces_done == count; NPOW_EXHAUSTED: nothing reached floor; NPOW_CANCELLED: the best candidate so
 * far and what was hashed; the nonce re-validated on the CPU; NPOW_ERR_INTERNAL rather than a possibly wrong answer;
 * a dropped device fails the job).  Every other ticket call refuses it as it refuses any best ticket,
 * npow_ticket_sweep and npow_promote included (a background best job cannot be lifted to a foreground one).
 * count == 0 completes at once (NPOW_EXHAUSTED).
 *
 * On each device the job's part is hashed only in launches built while no foreground job is live on that device or
 * waiting for it: searches from every other submit call, bounded searches, plain sweep jobs and plain best jobs are
 * foreground; background searches and background sweep jobs are not, and share a launch with the job.  While held out
 * the job keeps its slot, its generation, its place in the range and its best so far.  A launch that holds it takes
 * its span in chunks of 8,192 nonces per workgroup and ends within one chunk (~0.3 ms) once a foreground job arrives
 * or the launch's time budget (npow_set_pool_tuning) passes; what it did not reach goes back to the job, and what it
 * found stays a candidate.  It is admitted as background searches are: behind every waiting foreground job, under
 * the same cap on slots (at most half of them).
 * CONTINUOUS FOREGROUND LOAD STARVES IT: the job makes no progress while any foreground job is live on its devices,
 * for as long as that lasts.  That is the meaning of the class. */
int npow_submit_best_background(const uint8_t root[32], uint64_t floor, uint64_t start, uint64_t count,
                                uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket);

/* What its class cost an uncollected best job (npow_ticket_best_hold); npow_best_info keeps its size. */
typedef struct npow_best_hold_info {
  uint32_t size;          /* set by the caller; the library writes at most that many bytes */
  uint32_t background;    /* 1: npow_submit_best_background */
  uint64_t launches_cut;  /* launches that ended with part of their span unhashed: a yield or the time budget (the
                           * part went back to the job) */
  uint64_t held_us;       /* time the job sat admitted but left out of its devices' tables, summed over its devices */
} npow_best_hold_info;

/* The class of an uncollected best job's ticket, plain or background, and the launches cut and time held that came
 * with it (added within ABI 7; probe for the symbol); a plain best job reads 0, 0, 0.  Written up to out->size.
 * NPOW_ERR_BAD_ARGUMENT for any other kind of ticket, an unknown or collected one, or out / out->size missing.  Never
 * waits for a GPU. */
int npow_ticket_best_hold(uint64_t ticket, npow_best_hold_info* out);

/* Shared range jobs (added within ABI 7; probe for the symbols): a sweep job or a best job that takes a weighted
 * share of each GPU beside the searches -- the class between the plain one, whose launches no search can join or cut
 * short, and the background one, which continuous foreground load starves.  A shared job always makes progress, and a
 * search that arrives waits about one chunk of 8,192 nonces per workgroup (~0.3 ms), not a launch.
 *
 * The arguments, the split of the range over the GPUs of device_mask, the statuses and the guarantees are exactly
 * those of npow_submit_sweep / npow_submit_best (every nonce hashed exactly once; hits ascending by nonce - start and
 * *n_out exact, or the maximum of the range with the smallest nonce - start among equal values; a dropped device fails
 * the job; a cancel returns what was found).  npow_wait_sweep, npow_ticket_sweep, npow_wait_best, npow_ticket_best,
 * npow_ticket_best_hold and npow_cancel work on the ticket as they do on the plain job's; every other ticket call
 * returns NPOW_ERR_BAD_ARGUMENT and leaves it collectable.  count == 0 completes at once and touches no device.
 *
 * The job is admitted as a plain one is: a foreground job of weight 1 that takes a slot and counts against
 * npow_pool_config's limit.  Its entries are claimed ones, as the background class's: a launch takes its span in
 * chunks and gives the device back within one chunk once a search arrives or the launch's time budget passes; what it
 * did not reach goes back to the job.  But it is never held out of a table (held_us stays 0): the next launch holds the
 * search and the job.  Beside searches it weighs 1 in the launch's start map -- a weight-8 search beside it starts with
 * 8/9 of the workgroups -- and the workgroups of a search that ends early in a launch move to the job's chunks instead
 * of leaving the launch (npow_range_share_info.moves).  Background sweep and best jobs share its launches and are not
 * starved by it.  npow_sweep_info.background and npow_best_hold_info.background read 0 for it: the class is reported
 * by npow_ticket_share alone. */
int npow_submit_sweep_shared(const uint8_t root[32], uint64_t threshold, uint64_t start, uint64_t count,
                             uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket);
int npow_submit_best_shared(const uint8_t root[32], uint64_t floor, uint64_t start, uint64_t count,
                            uint64_t device_mask, const volatile uint32_t* cancel, uint64_t* ticket);

/* The class of an uncollected sweep or best job's ticket and what came with it (npow_ticket_share). */
typedef struct npow_range_share_info {
  uint32_t size;          /* set by the caller; written up to it */
  uint32_t klass;         /* 0 plain, 1 background, 2 shared */
  uint64_t launches;      /* launches that held an entry of the job, summed over its devices */
  uint64_t launches_cut;  /* of those, launches that ended with part of their span unhashed (claimed entries only) */
  uint64_t held_us;       /* time the job sat admitted but left out of its devices' tables (background jobs only) */
  uint64_t moves;         /* workgroups that came to the job's claimed entry from another entry of a running launch
                           * (counted in the kernel, read as each launch retires); 0 for plain jobs */
} npow_range_share_info;

/* Any sweep or best ticket (added within ABI 7; probe for the symbol).  Written up to out->size.
 * NPOW_ERR_BAD_ARGUMENT for a search's ticket, an unknown or collected one, or out / out->size missing.  Never waits
 * for a GPU. */
int npow_ticket_share(uint64_t ticket, npow_range_share_info* out);

/* Work values of `count` consecutive nonces start, start+1, ... for one root,
 * computed by the instruction stream the search and sweep kernels execute
 * (npow_values_kernel_ls2: the same uniform loads, priority runs and
 * workgroup shape), so the parity tests compare that stream's full 64-bit values
 * with the CPU.  device = logical device index. */
int npow_values(int device, const uint8_t root[32], uint64_t start, uint64_t count, uint64_t* values_out);

/* The same through a chosen hash path (NPOW_PATH_SEARCH = npow_values, NPOW_PATH_SEQ,
 * NPOW_PATH_GENERIC; the generic path takes count < 2^32). */
int npow_values_path(int device, const uint8_t root[32], uint64_t start, uint64_t count, int path,
                     uint64_t* values_out);

/* Work values of n independent (root_i, nonce_i) pairs on one device
 * (generic per-lane-root GPU path; server-side validation in bulk,
 * dpow_server.py:130,365). */
int npow_values_pairs(int device, const uint8_t* roots, const uint64_t* nonces, uint32_t n,
                      uint64_t* values_out);

/* Tuning knobs (0 keeps the current value).  iters_per_launch: the iteration cap of a
 * search launch (default 8192; a launch runs half as many wave iterations, each the time of two
 * hashes of another wave of its SIMD: 8 waves share it) and the span of bounded jobs' launches;
 * poll_interval: wave iterations between a wave's polls of the host kill / yield words
 * (rounded up to a power of two; 8 waves per iteration poll grid-wide at the default 1024);
 * blocks_per_cu: 256-lane workgroups per CU of the NPOW_PATH_SEQ values kernel. */
int npow_set_tuning(uint32_t iters_per_launch, uint32_t poll_interval, uint32_t blocks_per_cu);

/* Search (work pool) launches.  budget_us: wall-clock budget of a launch (default 20000;
 * 0 = iteration count only; 0xffffffff keeps the current value).  Workgroups searching unbounded
 * jobs stop together when it runs out -- VALU issue favours a SIMD's oldest wave, so a launch
 * of a fixed iteration count would end in a tail -- and iters_per_launch is then only the cap
 * (bounded jobs always complete their dense ranges).
 * The search kernel is npow_pool_kernel_ls2*: four 512-lane workgroups per CU, with
 * early finish (a won or cancelled job returns from the count its last workgroup publishes, not
 * at the end of the launch that held it) and dynamic entries (an unbounded job submitted while a
 * launch with other live jobs runs joins that launch).  A running launch is ended early (a yield)
 * only when a new job cannot join it: a bounded job, a one-job launch, a launch within 3 ms of its
 * budget, or a full ring of 32 dynamic entries.
 * blocks_per_cu: must be 0 or 4 (the workgroups per CU of the search kernel are fixed). */
int npow_set_pool_tuning(uint32_t budget_us, uint32_t blocks_per_cu);

/* Writes the ABI-2 prefix of npow_device_stats (through dyn_entries), as callers compiled
 * against that revision allocate. */
int npow_device_stats_get(int device, npow_device_stats* out);
/* Writes min(size, sizeof(npow_device_stats)) bytes. */
int npow_device_stats_get_sized(int device, npow_device_stats* out, uint64_t size);
int npow_device_stats_reset(int device);

/* Library / kernel identification string (gfx target, build flags). */
const char* npow_version(void);
/* NPOW_ABI_VERSION of the library. */
int npow_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* NANOPOW_H */
