/*
 * tcgpu.h -- C ABI of the MI355X-native batched GCRA engine (libtcgpu.so).
 *
 * This is the drop-in boundary for ONE hot path of lazureykis/throttlecrab:
 *     RateLimiter<AdaptiveStore>::rate_limit
 *         throttlecrab/src/core/rate_limiter.rs:102-250      (decision + advance)
 *         throttlecrab/src/core/rate/mod.rs:164-176          (emission interval)
 *         throttlecrab/src/core/store/mod.rs:85-133          (Store trait)
 *         throttlecrab/src/core/store/adaptive_cleanup.rs:138-279 (AdaptiveStore)
 * The reference has no FFI layer (it is 100 % Rust); the seam is the generic
 * `RateLimiter<S: Store>` that the server calls from
 *     throttlecrab-server/src/actor.rs:178-215 (StoreType::rate_limit).
 * A Rust maintainer binds these symbols with `extern "C"` (INTEGRATION.md
 * shows the stub) and gets `rate_limit` + the new `rate_limit_batch`.
 *
 * Semantics: a batch behaves EXACTLY as if its requests were applied one by
 * one, in index order, through the reference's `rate_limit` (duplicate keys
 * inside a batch included).  Integer results are bit-exact with the reference
 * inside the validated domain; outside it (where the reference panics or is
 * build-mode dependent) the request gets TC_INTERNAL and state is untouched:
 *     now_ns < 0                       (rate_limiter.rs:126-144 reads the wall clock)
 *     Duration * u32 overflow          (rate_limiter.rs:122 panics)
 *     now_ns + dvt overflows i64       (rate_limiter.rs:217 plain add)
 *
 * Ownership / threading: the handle is owned by the caller and is NOT
 * thread-safe (same contract as `&mut RateLimiter`, store/mod.rs:40-43): one
 * caller at a time; results are ordered on one HIP stream per engine (the
 * engine may group and stage batches on internal streams of its own).
 * Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Environment variables.  The library reads a number of TCGPU_* variables when an engine is created.  They are UNSUPPORTED TUNING
 * SWITCHES of the measurement scripts under tools/ (A/B of a kernel variant, a stream count, a threshold): none of them changes a
 * result, none is part of this ABI, any may disappear.  As of round 6:
 *   pipeline     TCGPU_AUX_STREAMS  TCGPU_PIPE_DEPTH  TCGPU_AUX_PRIORITY  TCGPU_PIPE_PROBE  TCGPU_ASSUME_CONCURRENT  TCGPU_STREAM_POOL
 *                TCGPU_STOP_EVENTS  TCGPU_PROF_MARKERS
 *   grouping     TCGPU_RANGE  TCGPU_RANGE_ILV  TCGPU_RANGE_MAX_N  TCGPU_SORT_ITEMS_PIPED  TCGPU_HOT  TCGPU_HOT_MIN  TCGPU_HOT_RANK  TCGPU_HOT_THREAD  TCGPU_BUCKET
 *                TCGPU_BUCKET_PIPED  TCGPU_BUCKET_BACKOFF  TCGPU_BUCKET_MIN_N  TCGPU_BUCKET_SKEW  TCGPU_ROUTE_3PASS
 *   evaluation   TCGPU_EVAL_ITEMS  TCGPU_EVAL_LEAN  TCGPU_PREFILL  TCGPU_GENERAL_EARLIER  TCGPU_GENERAL_RUNS  TCGPU_GENERAL_LEAN
 *                TCGPU_NO_SMALL_BATCH
 *   host batches TCGPU_HOST_CHUNK  TCGPU_BOUNCE_MAX  TCGPU_COPY_KERNEL  TCGPU_ASYNC_COPY_KERNEL_N  TCGPU_SYNC_COPY_MAX
 *   string keys  TCGPU_SPREAD_FREE  TCGPU_SWEEP_ASIDE        multi-GPU  TCGPU_EXCHANGE_WAIT_S
 * One more, TCGPU_DEBUG_NO_DECISION_STORE (the lean kernel skips its decision bytes: wrong results, for timing only), exists
 * only in libraries built with `make DEBUG_KNOBS=1` (-DTCGPU_DEBUG_KNOBS); the library this header ships with ignores it.
 */
#ifndef TCGPU_H
#define TCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCGPU_ABI_VERSION 1

typedef struct tc_engine tc_engine;

/* Per-request status = CellError (throttlecrab/src/core/mod.rs:49-56); 0 = Ok. */
enum {
    TC_OK = 0,
    TC_NEGATIVE_QUANTITY = 1,  /* CellError::NegativeQuantity  (rate_limiter.rs:111-113) */
    TC_INVALID_RATE_LIMIT = 2, /* CellError::InvalidRateLimit  (rate_limiter.rs:115-117) */
    TC_INTERNAL = 3            /* CellError::Internal          (outside validated domain) */
};

/* Call-level return codes (0 = success).  A negative return means the whole
 * call failed and NO request of the batch was applied -- except TC_E_TABLE_FULL:
 * the requests whose keys had or got a slot were applied, the others carry
 * status TC_INTERNAL. */
enum {
    TC_E_OK = 0,
    TC_E_INVALID_ARG = -1,
    TC_E_HIP = -2,            /* HIP runtime error; see tc_last_error().  Raised while a batch's inputs were being staged:
                               * nothing was applied and the engine is usable.  Raised by a RESULT copy (after the
                               * evaluation was enqueued): the batch was applied but its results are lost -- treat the
                               * engine as ahead of the caller (reload a snapshot, or drop it) */
    TC_E_NOMEM = -3,
    TC_E_BATCH_TOO_LARGE = -4,
    TC_E_TABLE_FULL = -5,     /* string mode: no free slot / arena space for a new key */
    TC_E_NO_DEVICE = -6,
    TC_E_UNSUPPORTED = -7,
    TC_E_AGAIN = -9,          /* tc_exchange_* with TC_X_NONBLOCKING: the phase's turn has not come (another rank, or the device,
                               * has to get further first); nothing was done, call again */
    TC_E_INVARIANT = -8       /* a kernel flagged a broken internal invariant (a wait on another workgroup gave up after
                               * 2 s, a closed form met a state it was proven not to meet): results and resident state
                               * since the last call that returned TC_E_OK from tc_synchronize() are UNDEFINED.  Sticky:
                               * every later call on the engine returns it; destroy the engine (reload a snapshot).
                               * Never seen unless there is a bug or the device lost forward progress. */
};

/* tc_config.flags */
#define TC_CFG_KEY_MODE 0x1u /* enable the on-device key->slot hash table (string keys) */
#define TC_CFG_TRACK_DENIED 0x2u /* keep a denial counter per key (4 B/slot) for tc_top_denied: the device-side
                                  * TopDeniedKeys of throttlecrab-server/src/metrics.rs:24-76 */

#define TC_CFG_FIXED_PARAMS 0x4u /* 8-byte resident state: one TAT per key instead of the 16-byte {tat, expiry} cell (half the
                                  * table, twice the keys per memory line).  Sound while a key's (burst, count, period)
                                  * never change -- then every write leaves expiry == tat + dvt (rate_limiter.rs:179-183,
                                  * adaptive_cleanup.rs:237) and the expiry column is redundant.  Hence, in this mode:
                                  *  - plans are registered BEFORE the first request (tc_register_params*; later calls
                                  *    return TC_E_UNSUPPORTED) and every batch carries TC_B_REGISTERED_PARAMS;
                                  *  - a plan needs burst >= 2 after the reference's `as u32` truncation and an emission
                                  *    interval / tolerance below 2^60 ns (else TC_E_UNSUPPORTED at registration);
                                  *  - timestamps >= 2^62 ns (year 2116) get TC_INTERNAL;
                                  *  - tc_rate_limit, the tc_store_* operations (free ttl) and TC_CFG_KEY_MODE (string
                                  *    keys carry their rate with every request) return TC_E_UNSUPPORTED.
                                  * Results and tc_read_state are bit-identical to the 16-byte layout otherwise. */

typedef struct tc_config {
    uint32_t struct_size;     /* = sizeof(tc_config) */
    uint32_t flags;           /* TC_CFG_* */
    int32_t device_id;        /* HIP device ordinal */
    int32_t reserved0;
    uint64_t capacity;        /* number of key slots resident in HBM */
    uint64_t max_batch;       /* largest n accepted by one rate_limit_batch call */
    uint64_t key_arena_bytes; /* string mode: overflow arena for keys longer than 112 bytes (shorter keys are
                               * stored inside their slot's 128-byte record); 0 = max(1 MiB, 4 B/slot) */
} tc_config;

/* tc_batch.flags */
#define TC_B_DEVICE_PTRS 0x1u       /* every pointer in the batch is a device pointer (async on the stream) */
#define TC_B_REGISTERED_PARAMS 0x2u /* use the per-slot (burst,count,period) set by tc_register_params */
#define TC_B_UNIQUE_SLOTS 0x4u      /* caller guarantees no slot occurs twice (skips grouping) */
#define TC_B_INPUTS_READY 0x8u      /* device-pointer batch whose `slot` column is already complete in device memory at
                                     * call time and stays untouched until the call's results are ready: the engine may
                                     * group (sort) it on an internal stream while earlier batches are still being
                                     * evaluated.  Evaluation order, results and visibility on the engine's stream are
                                     * unchanged; without the flag the whole batch runs in order on the engine's stream */

#define TC_B_GROUPED_OUTPUT 0x10u    /* write every output ROW in the order the engine evaluates in (grouped by key,
                                     * index order inside a key) and the request index of each row to `order`:
                                     * output row k belongs to request order[k].  Saves the engine one scattered
                                     * store per request; for consumers that walk all results anyway (a reply
                                     * fan-out).  Without the flag row i belongs to request i, as everywhere else. */

#define TC_B_OUTPUTS_IDLE 0x40u      /* with TC_B_INPUTS_READY: nothing enqueued before this call reads or writes the call's
                                     * output arrays (every batch in flight has arrays of its own, as a consumer that
                                     * reads results later needs anyway): the engine may initialise them on an internal
                                     * stream ahead of the evaluation.  Decisions-only batches then cost one store per
                                     * MINORITY decision instead of one per request.  Results are unchanged. */

/* One batch of requests = the argument list of RateLimiter::rate_limit
 * (rate_limiter.rs:102-110), columnar.  A NULL input column means "use the
 * scalar of the same name for every request". */
struct tc_decision;
#define TC_B_ASYNC 0x20u             /* HOST-pointer slot batch that only enqueues: the inputs are copied to the device,
                                     * evaluated and the outputs copied back asynchronously, overlapping the PCIe
                                     * transfers of one batch with the evaluation of others.  Input and output
                                     * arrays must stay untouched / are not valid until tc_wait_batches() says the
                                     * batch is done (or tc_synchronize()).  For the copies to be asynchronous the
                                     * arrays must be pinned (tc_host_alloc); with pageable memory the call is
                                     * correct but waits for its transfers.  Results are those of the in-order
                                     * sequence of calls, as always. */

#define TC_B_PLAN_DICT 0x80u         /* Round 6: the (max_burst, count_per_period, period) of every request as a 16-bit index into a
                                      * DICTIONARY the batch carries: plan_dict[n_plans][3] + plan_id[n] replace the three 8-byte
                                      * columns (which must be NULL), and quantity32[n], if given, replaces `quantity` -- 6 bytes per
                                      * request instead of 32.  A server's requests carry a handful of distinct triples; the
                                      * reference's signature rate_limit(key, max_burst, count_per_period, period, quantity, now)
                                      * (rate_limiter.rs:102-110) stays what the SHIMS take (Rust rate_limit_batch(&[Request]), the
                                      * C++ RateLimiter, the actor): they encode, falling back to the wide columns for a batch of more
                                      * than 65 536 distinct triples.  Same results as the wide form, request by request.  An index
                                      * >= n_plans decodes to (0, 0, 0): status TC_INVALID_RATE_LIMIT.  Host- and device-pointer
                                      * batches, slots and keys; not with TC_B_REGISTERED_PARAMS. */

typedef struct tc_batch {
    uint32_t struct_size; /* = sizeof(tc_batch) */
    uint32_t flags;       /* TC_B_* */
    uint64_t n;           /* number of requests */

    /* key: slots (tc_rate_limit_batch_slots) or a key arena (…_keys) */
    const uint32_t* slot;      /* [n] slot ids in [0, capacity) */
    const uint8_t* key_bytes;  /* key arena */
    const uint32_t* key_off;   /* [n+1] offsets into key_bytes */

    const int64_t* max_burst;        /* [n] or NULL */
    const int64_t* count_per_period; /* [n] or NULL */
    const int64_t* period;           /* [n] or NULL (seconds) */
    const int64_t* quantity;         /* [n] or NULL */
    const int64_t* now_ns;           /* [n] or NULL; SystemTime as ns since UNIX_EPOCH */
    int64_t max_burst_scalar;
    int64_t count_per_period_scalar;
    int64_t period_scalar;
    int64_t quantity_scalar;
    int64_t now_ns_scalar;

    /* outputs = (bool, RateLimitResult) (rate_limiter.rs:13-22) + status; any may be NULL */
    uint8_t* allowed;        /* [n] 0/1 */
    uint64_t* allowed_bits;  /* [(n+63)/64] bit i%64 of word i/64 = allowed[i] */
    int64_t* limit;          /* [n] */
    int64_t* remaining;      /* [n] */
    int64_t* reset_after_ns; /* [n] Duration as ns */
    int64_t* retry_after_ns; /* [n] Duration as ns */
    uint8_t* status;         /* [n] TC_OK / TC_NEGATIVE_QUANTITY / ... */
    /* RateLimitResult as ONE 32-byte record per request, {limit, remaining, reset_after_ns,
     * retry_after_ns}: a request's result then costs one scattered store instead of four
     * (use it instead of the four columns above when all fields are wanted). 16-byte aligned. */
    int64_t* result4;        /* [n][4] */
    struct tc_decision* decisions; /* [n] 32-byte records (see tc_decision below); 16-byte aligned */
    uint32_t* order;         /* [n] TC_B_GROUPED_OUTPUT: request index of each output row */

    /* A slot column that arrives in PIECES (tc_rate_limit_batch_slots, TC_B_DEVICE_PTRS): n_segments > 0 replaces
     * `slot` by seg_slot[0..n_segments) -- HOST arrays of device pointers and lengths, sum(seg_n) == n -- taken one
     * after the other: request i of the batch is the i-th entry of the concatenation.  What a shard of a multi-GPU
     * deployment receives: one segment per source GPU, in source order, so that a key's requests keep the order
     * of the global stream (tc_route_batch with only = -1 produces the segments).  The engine gathers the pieces on
     * the stream that groups the batch; with TC_B_INPUTS_READY every piece is complete in device memory at call time.
     * At most TC_MAX_SEGMENTS pieces. */
    uint32_t n_segments;
    uint32_t reserved_seg;
    const uint32_t* const* seg_slot; /* host array [n_segments] of device pointers */
    const uint32_t* seg_n;           /* host array [n_segments] */

    /* TC_B_PLAN_DICT (round 6; a tc_batch of an older struct_size simply ends before these) */
    const int64_t* plan_dict;   /* [n_plans][3]: max_burst, count_per_period, period (seconds) */
    const uint16_t* plan_id;    /* [n] index into plan_dict */
    const uint32_t* quantity32; /* [n] or NULL: the quantities as u32 (then `quantity` must be NULL) */
    uint32_t n_plans;           /* 1 .. 65536 */
    uint32_t reserved_dict;
} tc_batch;
#define TC_MAX_SEGMENTS 64

/* Everything rate_limit returns for one request except `limit` (== the request's max_burst, resp.
 * the key's registered burst), as ONE 32-byte record: a full result then costs a single scattered
 * store per request instead of three (result4 + allowed + status). */
typedef struct tc_decision {
    int64_t remaining;
    int64_t reset_after_ns;
    int64_t retry_after_ns;
    uint8_t allowed; /* 0/1 */
    uint8_t status;  /* TC_OK / TC_NEGATIVE_QUANTITY / ... */
    uint8_t pad[6];  /* zero */
} tc_decision;

/* What every transport of the reference answers with: ThrottleResponse {allowed, limit, remaining, reset_after, retry_after}
 * (throttlecrab-server/src/types.rs:74-96) -- the two durations in WHOLE SECONDS (Duration::as_secs(), types.rs:90-91) -- without
 * `limit` (the request's own max_burst), as ONE 16-byte record: half of tc_decision, one scattered store per request.
 * Every value has 34 bits, which makes the record exact rather than saturating:
 *   - a Duration the engine holds is i64 nanoseconds, so its seconds are < 2^63 / 10^9 < 2^34;
 *   - remaining = room / ei (rate_limiter.rs:217-225) with room <= now + dvt - cur and cur >= now - dvt (a live entry,
 *     :158-161) or cur = now - ei (a fresh one, quantity 0), so room <= max(2 dvt, dvt + ei).  dvt = ei * m with
 *     m = `(max_burst - 1) as u32` < 2^32 (:122): remaining <= max(2 m, 1) < 2^33.  Where ei * m does not fit i64 (dvt wraps), ei is
 *     at least 2^63 / 2^32 = 2^31 and room < 2^63, so remaining < 2^32.
 * So TC_T_WIDE is never set by this engine; the bit stays defined (a value >= 2^34 would store 2^34 - 1 and set it) so that a
 * reader need not trust this proof.  A status other than TC_OK gives all-zero values and allowed = 0. */
#define TC_T_WIDE 0x8u /* tc_throttle.bits: a value did not fit its 34 bits and was stored as 2^34 - 1 */
typedef struct tc_throttle {
    uint32_t remaining_lo;     /* low 32 bits of RateLimitResult::remaining */
    uint32_t reset_after_s_lo; /* low 32 bits of reset_after.as_secs() */
    uint32_t retry_after_s_lo; /* low 32 bits of retry_after.as_secs() */
    uint32_t bits;             /* bit 0 allowed | bits 1-2 status (TC_OK..TC_INTERNAL) | bit 3 TC_T_WIDE
                                * bits 8-9 remaining >> 32 | bits 10-11 reset_after_s >> 32 | bits 12-13 retry_after_s >> 32
                                * every other bit zero */
} tc_throttle;
/* (inline, not exported.  The names are parenthesised because the checks that compare this header's functions with the library's
 * exports and with the shims take every `tc_name(` for an exported symbol; call them as usual) */
static inline uint64_t (tc_throttle_remaining)(const tc_throttle* t) { return (uint64_t)t->remaining_lo | ((uint64_t)((t->bits >> 8) & 3u) << 32); }
static inline uint64_t (tc_throttle_reset_after_s)(const tc_throttle* t) { return (uint64_t)t->reset_after_s_lo | ((uint64_t)((t->bits >> 10) & 3u) << 32); }
static inline uint64_t (tc_throttle_retry_after_s)(const tc_throttle* t) { return (uint64_t)t->retry_after_s_lo | ((uint64_t)((t->bits >> 12) & 3u) << 32); }
static inline int (tc_throttle_allowed)(const tc_throttle* t) { return (int)(t->bits & 1u); }
static inline int (tc_throttle_status)(const tc_throttle* t) { return (int)((t->bits >> 1) & 3u); }

/* Single-request result (the tuple rate_limit returns). */
typedef struct tc_result {
    int64_t limit;
    int64_t remaining;
    int64_t reset_after_ns;
    int64_t retry_after_ns;
    uint8_t allowed;
    uint8_t status;
} tc_result;

/* Counter block (the payload all-gathered across GPUs; cf. the reference's
 * Metrics counters, throttlecrab-server/src/metrics.rs:84-94). */
enum {
    TC_CNT_TOTAL = 0,    /* requests decided */
    TC_CNT_ALLOWED = 1,
    TC_CNT_DENIED = 2,
    TC_CNT_ERRORS = 3,   /* status != TC_OK */
    TC_CNT_SWEPT = 4,    /* entries removed by tc_sweep_expired */
    TC_CNT_BATCHES = 5,
    TC_CNT_KEYS_INSERTED = 6,
    TC_CNT_LIVE_SLOTS = 7, /* the store's size, AdaptiveStore::len(): string mode -- the keys that hold a slot, exact in tc_counters();
                            * slot mode (and the device-resident block) -- occupied slots as of the last tc_sweep_expired */
    TC_CNT_COUNT = 8
};

uint32_t tc_abi_version(void);

/* RateLimiter::new(AdaptiveStore::with_capacity(..)) (rate_limiter.rs:56-58,
 * adaptive_cleanup.rs:93-106).  Returns NULL and sets *err on failure. */
tc_engine* tc_engine_create(const tc_config* cfg, int* err);
void tc_engine_destroy(tc_engine* e);

/* Issue all work on `hip_stream` (a hipStream_t) instead of the engine's own
 * stream; NULL restores the engine's stream. */
int tc_engine_set_stream(tc_engine* e, void* hip_stream);
/* Block until everything issued so far has finished. */
int tc_synchronize(tc_engine* e);
/* Message for the last negative return code (owned by the engine). */
const char* tc_last_error(const tc_engine* e);

/* Per-slot rate parameters kept as columns in HBM (emission interval, burst
 * tolerance, burst capacity).  slots == NULL registers slots [0, n).  Host
 * pointers.  Invalid parameter triples are rejected (TC_E_INVALID_ARG). */
int tc_register_params(tc_engine* e, uint64_t n, const uint32_t* slots, const int64_t* max_burst,
                       const int64_t* count_per_period, const int64_t* period);
/* Same triple for every slot. */
int tc_register_params_uniform(tc_engine* e, int64_t max_burst, int64_t count_per_period, int64_t period);

/* rate_limit_batch over pre-resolved slots / over string keys.
 * Host-pointer batches return after the results are in the output arrays (up to 1024 requests are served by
 * one kernel launch, ~30-40 us per call; larger ones by the grouping + evaluation pipeline), unless flagged
 * TC_B_ASYNC; TC_B_DEVICE_PTRS batches are asynchronous on the engine's stream. */
int tc_rate_limit_batch_slots(tc_engine* e, const tc_batch* b);
int tc_rate_limit_batch_keys(tc_engine* e, const tc_batch* b);
/* The same two calls with one more output: out[i] (a tc_throttle record, 16-byte aligned; host or device memory as b->flags
 * says, like every other array of the batch) answers request i -- row k answers request order[k] under TC_B_GROUPED_OUTPUT.
 * Every flag and input form of tc_batch means what it means above, the other output pointers of `b` may be set as well and
 * are written as before; a batch that asks for these records is evaluated with full results.  out == NULL or misaligned:
 * TC_E_INVALID_ARG, nothing is applied.  16 bytes come back per request instead of tc_decision's 32, for a transport that
 * answers in whole seconds anyway (types.rs:86-94, transport/grpc.rs:183-189).  `out` points at tc_throttle[n].  It is declared
 * void*, at the price of the compiler's check on it, because the check that holds the Rust shim to this header
 * (tests/test_rust_shim.py) translates parameter types through a closed list of type names. */
int tc_throttle_batch_slots(tc_engine* e, const tc_batch* b, void* out);
int tc_throttle_batch_keys(tc_engine* e, const tc_batch* b, void* out);

/* ---- read-only batch queries ------------------------------------------------------------------------------------------------
 * The reference cannot look at a limiter without changing it: a request with quantity 0 stores the clamped TAT and a new TTL on a
 * known key (rate_limiter.rs:158-195), INSERTS an unknown one (set_if_not_exists_with_ttl) and counts as a store operation.  A
 * dashboard, a quota display or an admission pre-check over a million string keys would bind a million slots.  These two calls
 * answer a batch and change nothing.
 *   Answer i is what rate_limit(key_i, max_burst_i, count_per_period_i, period_i, quantity_i, now_i) would return if it were the
 *   NEXT AND ONLY request, given the state every earlier call on the engine has left: the reference's arithmetic on a copy of the
 *   key's entry, the copy thrown away.  An unknown key, an unbound or never-written slot and an entry with expiry <= now_i are
 *   the reference's "first request" branch (rate_limiter.rs:162-166).  The requests of one peek do not see one another:
 *   duplicates get identical answers.  Validation and the precedence of the statuses are those of the batch calls; a status other
 *   than TC_OK gives all-zero values and allowed = 0.
 *   NOTHING CHANGES: no cell; no key-table entry (nothing claimed, no tombstone recycled, no slot taken, free stack and overflow
 *   arena as they were); no TC_CNT_* counter (TC_CNT_BATCHES included); no denial counter, no retired key; the cleanup policy's
 *   operation count does not move and a peek never triggers a sweep; no grouping hint, no hot list.  On a TC_CFG_FIXED_PARAMS
 *   engine a peek before the first batch does NOT seal the plans -- it decides nothing -- so tc_register_params* still work
 *   after it.
 *   Outputs: any of b->decisions (tc_decision[n]), b->allowed, b->status and `out` (tc_throttle[n], 16-byte aligned, or NULL) that
 *   are given are written, row i for request i; at least one must be.  Any OTHER output pointer of `b` being set: TC_E_INVALID_ARG.
 *   `out` is declared void* for the reason tc_throttle_batch_* give above.
 *   Inputs: every form tc_batch has -- scalars or columns; TC_B_PLAN_DICT with quantity32; for slots TC_B_REGISTERED_PARAMS
 *   (mandatory on a TC_CFG_FIXED_PARAMS engine, as for batches; a slot out of range gets TC_INTERNAL, as there); host pointers
 *   (pinned or pageable: staged, run, copied back -- the call returns with the answers) or TC_B_DEVICE_PTRS (asynchronous on the
 *   engine's stream).  n = 1 .. max_batch (n = 0: TC_E_OK, nothing to answer).  TC_B_INPUTS_READY and TC_B_OUTPUTS_IDLE are
 *   accepted and mean nothing.  TC_B_ASYNC, TC_B_GROUPED_OUTPUT, TC_B_UNIQUE_SLOTS and n_segments > 0: TC_E_UNSUPPORTED.
 *   tc_peek_batch_keys on an engine without TC_CFG_KEY_MODE: TC_E_UNSUPPORTED.  A refused call enqueues nothing.
 *   Ordering: a peek sees every batch, sweep and store operation whose call returned before it -- pipelined ones included, whose
 *   key stages run on a stream of the engine's own -- and nothing of the calls made after it: it is one kernel on the engine's
 *   stream, behind the last key stage, and the key stage, sweep or table rebuild of a later call does not start before it has
 *   finished reading.  No host synchronisation is involved for device-pointer peeks.
 *   Cost: one launch, one lane per request: hash, probe, confirm, one 16-byte cell read, one 16-byte record written. */
int tc_peek_batch_keys(tc_engine* e, const tc_batch* b, void* out);
int tc_peek_batch_slots(tc_engine* e, const tc_batch* b, void* out);

/* TC_B_ASYNC batches: block until at most `max_in_flight` of them are still incomplete (0 = all done).
 * A caller that cycles through K sets of pinned buffers calls tc_wait_batches(e, K - 1) before it
 * refills the oldest set.  (The reference's actor answers one request per loop turn,
 * throttlecrab-server/src/actor.rs:217-236; this is what lets a batch-draining actor fill the next
 * batch while the previous ones are in flight.) */
int tc_wait_batches(tc_engine* e, uint32_t max_in_flight);
/* Pinned host memory (hipHostMalloc / hipHostFree behind a C signature): what TC_B_ASYNC batches need, and what makes a
 * synchronous host-pointer batch fastest -- its arrays cross PCIe in one copy launch each way, and from 512 Ki requests on the
 * batch is pipelined in chunks.  Arrays in pageable memory are always correct: up to 4 MB of them per call go through a pinned
 * block of the engine's own (two memcpys by the calling thread), larger ones through the runtime's staging copies. */
void* tc_host_alloc(size_t bytes);
void tc_host_free(void* p);

/* RateLimiter::rate_limit (rate_limiter.rs:102-250), one request, string key.
 * Returns 0 and fills *out (out->status carries the CellError). */
int tc_rate_limit(tc_engine* e, const uint8_t* key, size_t key_len, int64_t max_burst,
                  int64_t count_per_period, int64_t period, int64_t quantity, int64_t now_ns,
                  tc_result* out);

/* AdaptiveStore::cleanup (adaptive_cleanup.rs:173-203): drop every entry with
 * expiry <= now.  Decision-neutral.  removed == NULL: the sweep is only enqueued on the
 * engine's stream (no host wait; the number removed is added to TC_CNT_SWEPT). */
int tc_sweep_expired(tc_engine* e, int64_t now_ns, uint64_t* removed);

/* ---- self-cleaning: AdaptiveStore::maybe_clean_expired behind the engine's own calls -----------------------------------
 * The reference's stores clean THEMSELVES: every compare_and_swap_with_ttl / set_if_not_exists_with_ttl first runs
 * maybe_clean_expired (adaptive_cleanup.rs:205-211,229,262; periodic.rs:128-142; probabilistic.rs:110-125), so a
 * `RateLimiter<AdaptiveStore>` never fills up with expired keys.  With a policy set, the engine does the same in front of
 * every mutating call (tc_rate_limit, tc_rate_limit_batch_keys / _slots, tc_store_compare_and_swap_with_ttl,
 * tc_store_set_if_not_exists_with_ttl): it counts the reference's operations (one per allowed request / store call), looks
 * at the call's timestamp and at the store's size and, when the reference's should_clean would say yes, enqueues
 * tc_sweep_expired at that timestamp in front of the call -- on the engine's stream, nothing waits.  A batch is one step:
 * the trigger is evaluated once per call with the call's first timestamp, where the reference evaluates it per request.
 * Cleanup never changes a decision while timestamps do not decrease, so results stay bit-exact.
 * String mode adds what a fixed-size table needs where the reference's HashMap would grow:
 *   - room: a key batch that might not find n free slots is preceded by a sweep (and, if the numbers the host holds are
 *     older than that sweep, by one wait for fresh ones);
 *   - retry: a SYNCHRONOUS call that still ran out of slots (TC_E_TABLE_FULL) sweeps at the newest timestamp of the call and
 *     applies the rejected requests once more, in order, before it reports the error.
 * Without a policy (the default of tc_engine_create) the engine never cleans by itself: tc_sweep_expired is the
 * caller's.  The host mirrors (throttlecrab_gpu.hpp GpuStore, rust/throttlecrab-gpu) set TC_SWEEP_ADAPTIVE with the
 * server's defaults (throttlecrab-server/src/config.rs:285-304) when they create their engine. */
enum {
    TC_SWEEP_NONE = 0,
    TC_SWEEP_ADAPTIVE = 1,      /* adaptive_cleanup.rs:138-211 */
    TC_SWEEP_PERIODIC = 2,      /* periodic.rs:128-142 */
    TC_SWEEP_PROBABILISTIC = 3  /* probabilistic.rs:110-125 */
};
typedef struct tc_sweep_policy {
    uint32_t struct_size;         /* = sizeof(tc_sweep_policy) */
    uint32_t kind;                /* TC_SWEEP_* */
    int64_t created_ns;           /* the store's creation time (`SystemTime::now()` in with_capacity): the first time-based
                                   * cleanup is due one interval later (adaptive: 5 s, DEFAULT_CLEANUP_INTERVAL_SECS) */
    int64_t min_interval_ns;      /* adaptive; 0 = 1 s (MIN_CLEANUP_INTERVAL_SECS; the server's default is 5 s) */
    int64_t max_interval_ns;      /* adaptive; 0 = 300 s */
    int64_t interval_ns;          /* periodic; 0 = 60 s */
    uint64_t max_operations;      /* adaptive; 0 = 100 000 (MAX_OPERATIONS_BEFORE_CLEANUP; the server's default is 1 000 000) */
    uint64_t map_capacity;        /* adaptive: the `capacity` of AdaptiveStore::with_capacity -- the memory-pressure trigger
                                   * fires above 3/4 of 1.3 x this many entries; 0 = the engine's capacity / 1.3, i.e. the
                                   * trigger fires when 3/4 of the engine's slots are taken */
    uint64_t cleanup_probability; /* probabilistic; 0 = 1000 */
} tc_sweep_policy;
/* p == NULL or kind == TC_SWEEP_NONE: the engine stops cleaning by itself. */
int tc_set_sweep_policy(tc_engine* e, const tc_sweep_policy* p);
typedef struct tc_sweep_info {
    uint32_t struct_size;          /* = sizeof(tc_sweep_info), set by the caller */
    uint32_t kind;                 /* the policy in force */
    uint64_t sweeps;               /* sweeps the engine started by itself since the policy was set ... */
    uint64_t sweeps_by_time;       /* ... because the interval had passed (adaptive_cleanup.rs:140, periodic.rs:129) */
    uint64_t sweeps_by_operations; /* ... the operation count (:145) or the probabilistic draw (probabilistic.rs:116) */
    uint64_t sweeps_by_size;       /* ... the size of the store (:150-168) */
    uint64_t sweeps_for_room;      /* ... a key batch that might not have found free slots */
    uint64_t retries;              /* synchronous calls that ran out of slots, swept and applied the rejected requests again */
    uint64_t feed_waits;           /* times a call waited for fresh numbers from the device (room checks only) */
    uint64_t operations;           /* operations counted since the last cleanup */
    uint64_t entries;              /* the store's size as the host last saw it (string mode: bound keys) */
    uint64_t last_removed;         /* entries the last cleanup the host has heard of removed */
    int64_t current_interval_ns;   /* adaptive: current_cleanup_interval */
    int64_t next_cleanup_ns;       /* adaptive / periodic: next_cleanup */
} tc_sweep_info;
int tc_sweep_stats(tc_engine* e, tc_sweep_info* out);

/* Copy the counter block to host (refreshes it first). */
int tc_counters(tc_engine* e, uint64_t out[TC_CNT_COUNT]);
/* Fold the engine's sharded decision counters into the device-resident counter
 * block (asynchronous on the stream).  Call before reading the block through
 * tc_counters_device_ptr, e.g. right before the RCCL all-gather. */
int tc_counters_refresh(tc_engine* e);
/* Per-stage timing of the batch pipeline with HIP events recorded on the
 * engine's stream between its kernels (diagnostics for the roofline report;
 * leave off in production -- every event is an extra stream operation). */
enum {
    TC_STAGE_PREP = 0,   /* digit histograms of the batch (rs::k_hist) */
    TC_STAGE_SORT = 1,   /* one radix pass (rs::k_onesweep); counted once per pass */
    TC_STAGE_EVAL = 2,   /* GCRA decide + advance */
    TC_STAGE_COMMIT = 3, /* deferred cell stores */
    TC_STAGE_PACK = 4,   /* decision bit packing */
    TC_STAGE_HASH = 5,   /* string mode: key -> slot resolution */
    /* uniform batches are grouped WITHOUT a sort when their keys are spread evenly (bucket path): */
    TC_STAGE_BUCKET_HIST = 6,    /* requests per key-range bucket, per 4096-request tile (bp::k_tile_hist) */
    TC_STAGE_BUCKET_SCAN = 7,    /* prefix of those counts over the tiles (bp::k_bucket_scan) */
    TC_STAGE_BUCKET_SCATTER = 8, /* stable partition of the batch by bucket (bp::k_scatter) */
    TC_STAGE_BUCKET_EVAL = 9,    /* rank + GCRA decide + advance, one wave per bucket (bp::k_bucket_eval) */
    TC_STAGE_COUNT = 10
};
int tc_profile_enable(tc_engine* e, int on);
/* Accumulated milliseconds and launches per stage since tc_profile_enable. */
int tc_profile_read(tc_engine* e, double total_ms[TC_STAGE_COUNT], uint64_t calls[TC_STAGE_COUNT]);

/* Device address of the counter block (uint64[TC_CNT_COUNT]) for an on-device
 * collective (RCCL all-gather) without a host round trip. */
int tc_counters_device_ptr(tc_engine* e, void** dptr);

/* `trait Store` parity shims (store/mod.rs:85-133), one key per call. */
int tc_store_get(tc_engine* e, const uint8_t* key, size_t key_len, int64_t now_ns, int64_t* value, int* found);
int tc_store_compare_and_swap_with_ttl(tc_engine* e, const uint8_t* key, size_t key_len, int64_t old_value,
                                       int64_t new_value, uint64_t ttl_ns, int64_t now_ns, int* swapped);
int tc_store_set_if_not_exists_with_ttl(tc_engine* e, const uint8_t* key, size_t key_len, int64_t value,
                                        uint64_t ttl_ns, int64_t now_ns, int* was_set);

/* Introspection for differential tests: raw (tat, expiry) columns of slots
 * [first, first+n) copied to host.  expiry is ns since epoch saturated to u64;
 * 0 = vacant. */
int tc_read_state(tc_engine* e, uint64_t first, uint64_t n, int64_t* tat, uint64_t* expiry);
/* string mode: slot currently bound to `key`, or -1. */
int tc_lookup_slot(tc_engine* e, const uint8_t* key, size_t key_len, int64_t* slot);

/* Top denied keys (metrics.rs:24-76,296-309: `throttlecrab_top_denied_keys{key,rank}`).  Needs
 * TC_CFG_TRACK_DENIED.  Counts are exact (the reference's capped HashMap forgets keys when it
 * overflows).  Slot mode: a slot IS the key.  Key mode: this call reports the keys that currently
 * hold a slot; tc_top_denied_keys also knows the keys a sweep has unbound (the reference counts by
 * key, whatever its store cleans up).  Returns the k slots with the most denials since creation / tc_denied_reset,
 * most denied first (ties: lower slot first), k is capped at 10 000 like the reference's
 * MAX_DENIED_KEYS_LIMIT; slots never denied are not listed.  *n_out <= k entries are written. */
int tc_top_denied(tc_engine* e, uint32_t k, uint32_t* slots, uint64_t* counts, uint32_t* n_out);
int tc_denied_reset(tc_engine* e);
/* string mode: TopDeniedKeys::get_top (metrics.rs:66-76) -- the k most denied KEYS, most denied first (ties: key
 * bytes ascending), as a key arena (key_off[k + 1]) + counts.  A key's denials follow the key: a sweep that unbinds it
 * moves the count into a side table of 65 536 keys (keys of up to 256 bytes, the reference's MAX_KEY_LENGTH; trimmed
 * to the 10 000 most denied ones once it passes 30 000, like TopDeniedKeys::cleanup), and binding the key again
 * moves it back.  k is capped at 10 000.  TC_E_INVALID_ARG if key_bytes_cap is too small. */
int tc_top_denied_keys(tc_engine* e, uint32_t k, uint8_t* key_bytes, size_t key_bytes_cap, uint32_t* key_off, uint64_t* counts,
                       uint32_t* n_out);
/* string mode: the keys bound to `slots` as an arena (key_off[n+1]); an unbound slot yields an
 * empty key.  TC_E_INVALID_ARG if key_bytes_cap is too small. */
int tc_slot_keys(tc_engine* e, uint32_t n, const uint32_t* slots, uint8_t* key_bytes, size_t key_bytes_cap,
                 uint32_t* key_off);

/* ---- multi-GPU: routing a global request stream to the GPU that owns each key -----------------------------
 * The reference has no distributed mode ("use client-side sharding by key", README.md:247-249).  A key space of
 * world * keys_per_shard GLOBAL ids is sharded without a routing table by a bijection of that range:
 *     q = id div world, r = id mod world:   shard-local slot = q,   owner = (r + mix(q)) mod world
 * (mix(q) = the top bits of q * 0x9E3779B1 scaled to [0, world): ids that share a residue are still spread over all
 * owners) -- every shard gets exactly keys_per_shard dense slots.  tc_route_batch keeps, of a batch of global ids
 * in device memory, the requests a destination owns (stable: the requests of a key keep their order) as
 * shard-local slots ready for tc_rate_limit_batch_slots; asynchronous on the engine's stream (or on r->stream).
 * No collective is involved: each GPU filters the stream it is handed. */
/* tc_route.flags */
#define TC_ROUTE_AHEAD 0x1u   /* run the router on one of the engine's grouping streams, ordered behind the grouping of
                               * every batch whose call has returned (the last reader of a slot column -- except for
                               * TC_B_UNIQUE_SLOTS batches, whose evaluation reads it -- so out_slot may be a buffer an
                               * earlier batch call was given); successive routers rotate over those streams and do
                               * not wait for one another (give each its own out_* buffers): it then
                               * works beside the evaluations of earlier batches instead of between them -- with
                               * out_count_host, the way to route several global batches ahead of the evaluation */
#define TC_ROUTE_NO_READERS 0x2u /* with TC_ROUTE_AHEAD: out_slot is not the slot column of any batch still in flight (the
                               * caller forwards the segments elsewhere, tc_forward_segments): the router waits for nothing */
typedef struct tc_route {
    uint32_t struct_size;     /* = sizeof(tc_route) */
    uint32_t world;           /* number of shards (GPUs), 1..64 */
    uint64_t keys_per_shard;  /* slots of every shard (the engines' capacity) */
    uint64_t n;               /* requests in the global batch (<= the engine's max_batch * world) */
    const uint32_t* global_id; /* [n] device: global key ids in [0, world * keys_per_shard) (others: taken modulo) */
    int32_t only;             /* >= 0: write that destination's requests only, from out_slot[0];
                               * -1: every destination's segment, one after the other (start of d = sum of counts before d) */
    uint32_t flags;           /* TC_ROUTE_* */
    uint32_t* out_slot;       /* [n] device: shard-local slots */
    uint32_t* out_pos;        /* [n] device or NULL: position of each kept request in the global batch */
    uint32_t* out_count;      /* [world] device: requests per destination (all of them, whatever `only` is) */
    void* stream;             /* NULL: the engine's stream.  Else the hipStream_t to enqueue the router on (the caller
                               * orders that stream before the batch call that reads out_slot; successive
                               * tc_route_batch calls must use one stream) */
    uint32_t* out_count_host; /* NULL or [world + 1] PINNED host memory (tc_host_alloc): the router's last block
                               * writes the counts there and, after them, `tag` into out_count_host[world].  A caller
                               * that polls that word needs no stream synchronisation to learn how many requests it
                               * owns: once the tag is there, out_slot / out_pos are complete too. */
    uint32_t tag;             /* any value the previous use of out_count_host did not leave there */
    uint32_t reserved1;
    uint32_t* const* out_dst; /* NULL, or (only == -1) a HOST array [world] of device pointers: segment d is written to
                               * out_dst[d], from its start, instead of into out_slot (which may then be NULL; out_pos is
                               * not written) -- out_dst[d] is the inbox destination d keeps for this source, in d's own
                               * memory (peer memory over xGMI, hipIpcOpenMemHandle): routing and forwarding in one pass.
                               * Once out_count_host carries the tag, every segment has landed. */
} tc_route;
int tc_route_batch(tc_engine* e, const tc_route* r);
/* The exchange step of a sharded deployment in which every GPU routes only ITS slice of the global stream
 * (tc_route_batch with only = -1: one segment per destination, one after the other in out_slot): copy segment d to
 * dst[d] -- the inbox the destination keeps for this source, in its own memory (peer memory over xGMI, mapped
 * through hipIpcOpenMemHandle; dst[own rank] is local) -- in ONE launch on `stream` (NULL: the engine's stream).
 * count[] is the host copy of tc_route.out_count (out_count_host).  Peer copies, no collective: the decision path
 * of the reference has none either (README.md:247-249 shards on the client).  The destination evaluates the
 * inboxes of a step as one batch with a segmented slot column (tc_batch.seg_slot), sources in rank order. */
typedef struct tc_forward {
    uint32_t struct_size;      /* = sizeof(tc_forward) */
    uint32_t world;            /* 1..64 */
    const uint32_t* src;       /* device: the router's out_slot */
    const uint32_t* count;     /* HOST [world]: requests per destination */
    uint32_t* const* dst;      /* HOST [world]: device pointers, dst[d] has room for count[d] entries */
    void* stream;              /* hipStream_t or NULL */
} tc_forward;
int tc_forward_segments(tc_engine* e, const tc_forward* f);

/* ---- the exchange as library calls (one rank's side; `--route exchange` of bench.py) -----------------------------------
 * Every rank owns `ring` inbox slots per source in its own HBM ([ring][world][seg_cap] u32, shared with the peers through
 * hipIpcGetMemHandle / hipIpcOpenMemHandle once, at set-up) and the ranks share one small host-memory block: mail
 * [world][ring][world][2] = (count, step + 1) written by a source once its segment has landed, and done[world] = steps a
 * destination has evaluated (which frees its inbox slots).  Per step i a rank
 *   routes   its slice of global step i + route_ahead straight into the owners' inboxes (tc_route_batch, only = -1, out_dst),
 *   posts    step i + post_ahead: (count, step) into every destination's mailbox once the router's tag is in,
 *   collects the world mailbox words of step i and
 *   evaluates the world inboxes as ONE batch whose slot column comes in pieces (sources in rank order).
 * tc_exchange_step is those four in one call.  No collective, no host synchronisation in steady state (a phase only waits
 * when its inputs are not there yet).  The caller primes the pipeline: routes 0 .. route_ahead - 1, posts 0 .. post_ahead - 1.
 * tmpl: outputs, rate plan / quantity / timestamp and flags of the evaluation (device pointers; TC_B_INPUTS_READY is added);
 * a step larger than the engine's max_batch is evaluated in chunks, each writing behind the previous one.  tmpl->n, if not 0, is
 * the number of requests the output arrays hold: a step (tc_shard_evaluate: this rank's share of it) that is larger fails with
 * TC_E_INVALID_ARG before anything is applied.  */
#define TC_X_NONBLOCKING 0x1u    /* a phase whose turn has not come returns TC_E_AGAIN instead of waiting (ONE thread driving
                                  * several ranks, as the tests do); a repeated phase of a step already done is a no-op */
typedef struct tc_exchange tc_exchange;
typedef struct tc_exchange_config {
    uint32_t struct_size;      /* = sizeof(tc_exchange_config) */
    uint32_t rank;             /* this shard */
    uint32_t world;            /* shards, 1..64 */
    uint32_t ring;             /* inbox slots per source (>= 2; a source may run ring - 1 steps ahead of a destination) */
    uint32_t seg_cap;          /* requests one source may send per step (the slice length) */
    uint32_t flags;            /* TC_X_* */
    uint64_t keys_per_shard;
    uint32_t* const* inbox;    /* HOST array [world]: inbox[d] = destination d's [ring][world][seg_cap] array as THIS process
                                * addresses it (own: device memory; peers: hipIpcOpenMemHandle) */
    uint32_t* mail;            /* host memory shared by all ranks, zero at set-up: [world][ring][world][2] */
    int64_t* done;             /* ... [world] */
} tc_exchange_config;
/* (an exchange points into its engine: destroy it first.  A step may be routed at most 8 steps ahead of its post.) */
int tc_exchange_create(tc_engine* e, const tc_exchange_config* c, tc_exchange** out);
int tc_exchange_destroy(tc_exchange* x);
int tc_exchange_route(tc_exchange* x, uint64_t step, const uint32_t* global_id, uint32_t n);
int tc_exchange_post(tc_exchange* x, uint64_t step);
int tc_exchange_collect(tc_exchange* x, uint64_t step, uint32_t* counts /* [world] or NULL */);
int tc_exchange_evaluate(tc_exchange* x, uint64_t step, const tc_batch* tmpl, uint64_t* decided);
int tc_exchange_step(tc_exchange* x, uint64_t step, const uint32_t* global_id_ahead, uint32_t n_ahead, uint32_t route_ahead,
                     uint32_t post_ahead, const tc_batch* tmpl, uint64_t* decided);
/* publish the steps whose evaluation has completed (frees inbox slots for the sources); never waits */
int tc_exchange_poll(tc_exchange* x);
/* host time (ns) the calls have spent WAITING since the last call of this function: [0] for free inbox slots (route), [1] for
 * the router's tag (post), [2] for the sources' mailbox words (collect) -- what tells a host-bound step from a starved one */
int tc_exchange_wait_ns(tc_exchange* x, uint64_t out[3]);

/* ---- `replicate` mode as library calls (one rank's side; bench.py --route replicate) -------------------------------------------
 * Every rank is handed the WHOLE global batch; per step i it
 *   routes    global step i + route_ahead: keeps what it owns as shard-local slots (tc_route_batch, one destination) on one of the
 *             engine's grouping streams, beside the evaluations, into one of `ring` columns of its own; the router's last block
 *             leaves the counts and the step's tag in pinned host memory,
 *   evaluates step i: polls that tag (routed a few steps ago: no wait in steady state), and decides its share -- in batches of
 *             at most max_batch, each writing its outputs behind the previous one's.
 * tc_shard_step is both in one call: a rank's host cost per step is one call (round 4: four Python calls, 26-38 us).  The caller
 * primes the pipeline: routes steps 0 .. route_ahead - 1.  tmpl: as for tc_exchange_evaluate.  No collective, no peer memory. */
typedef struct tc_shard tc_shard;
typedef struct tc_shard_config {
    uint32_t struct_size;     /* = sizeof(tc_shard_config) */
    uint32_t rank;            /* this shard */
    uint32_t world;           /* shards, 1..64 */
    uint32_t ring;            /* routed batches kept (>= route_ahead + 2, at most 64) */
    uint64_t keys_per_shard;  /* the engines' capacity */
    uint64_t max_global;      /* requests of the largest global batch */
} tc_shard_config;
/* (a shard points into its engine: destroy it first) */
int tc_shard_create(tc_engine* e, const tc_shard_config* c, tc_shard** out);
int tc_shard_destroy(tc_shard* x);
int tc_shard_route(tc_shard* x, uint64_t step, const uint32_t* global_id, uint64_t n);
int tc_shard_evaluate(tc_shard* x, uint64_t step, const tc_batch* tmpl, uint64_t* decided);
int tc_shard_step(tc_shard* x, uint64_t step, const uint32_t* global_id_ahead, uint64_t n_ahead, uint32_t route_ahead, const tc_batch* tmpl,
                  uint64_t* decided);
/* host time (ns) the calls have spent waiting for a router's tag since the last call of this function */
int tc_shard_wait_ns(tc_shard* x, uint64_t* out);

/* The same map on the host: owner and shard-local slot of n global ids (either output may be NULL), and its
 * inverse (global id of slot `slot` of shard `owner`).  No device needed. */
int tc_route_host(uint32_t world, uint64_t keys_per_shard, uint64_t n, const uint32_t* global_id, uint32_t* owner,
                  uint32_t* slot);
int tc_route_inverse(uint32_t world, uint64_t keys_per_shard, uint64_t n, const uint32_t* owner, const uint32_t* slot,
                     uint64_t* global_id);

/* String keys across GPUs (README.md:247-249: "client-side sharding by key"): owner[i] = mix64(hash(key i) ^ salt) mod world --
 * the front door of a sharded deployment of key-mode engines: split a key batch by owner, hand every GPU the keys it owns.
 * key_off[n + 1] delimits the keys in key_bytes.  Host only. */
int tc_route_keys_host(uint32_t world, uint64_t n, const uint8_t* key_bytes, const uint32_t* key_off, uint32_t* owner);
/* The same split on the device: a key batch that is already in device memory (staged from the host, or handed on by the peer GPU
 * that took the connection) is partitioned by owner -- the owner map above, bit for bit -- into one arena per destination.
 * Stable: the keys of a destination keep the order they had in the batch, so a key's requests keep theirs; empty keys are keys.
 * only == -1: segment d holds count_d keys and bytes_d bytes; with start_d = the counts before d and bstart_d = the bytes before d,
 *   its bytes are out_bytes + bstart_d, its count_d + 1 offsets are out_off[start_d + d ..] (relative to its own bytes: the first is
 *   0, the last bytes_d) and the positions its keys had in the batch are out_pos[start_d ..]: (out_bytes + bstart_d,
 *   out_off + start_d + d, count_d) is a complete arena for tc_rate_limit_batch_keys / tc_throttle_batch_keys (TC_B_DEVICE_PTRS) on
 *   this GPU, or for a copy to a peer.
 * only >= 0: that destination's segment alone, at out_bytes, out_off[0 .. count], out_pos[0 .. count).
 * Nothing beyond that layout is written.  Works on any engine, key mode or not (the key table is not touched); asynchronous on
 * `stream`.  key_off must not decrease.  Three launches, none of which waits for another workgroup.  A bad world, n, only, flags
 * or a NULL array: TC_E_INVALID_ARG, nothing is enqueued. */
typedef struct tc_key_route {
    uint32_t struct_size;      /* = sizeof(tc_key_route) */
    uint32_t world;            /* 1..64 */
    uint64_t n;                /* keys in the batch, 1 .. 2^31 - 1 */
    const uint8_t* key_bytes;  /* device: the arena */
    const uint32_t* key_off;   /* device [n + 1] */
    int32_t only;              /* >= 0: that destination's keys only, from the start of the outputs; -1: every destination's segment */
    uint32_t flags;            /* must be 0 */
    uint8_t* out_bytes;        /* device, room for key_off[n] bytes */
    uint32_t* out_off;         /* device [n + world] */
    uint32_t* out_pos;         /* device [n] or NULL: position of every kept key in the input batch */
    uint32_t* out_count;       /* device [2 * world]: keys per destination, then bytes per destination (all of them, whatever `only` is) */
    void* stream;              /* NULL: the engine's stream.  Else the hipStream_t to enqueue the router on */
    uint32_t* out_count_host;  /* NULL or PINNED host memory [2 * world + 1] (tc_host_alloc): the same numbers, then `tag`, written last */
    uint32_t tag;              /* any value the previous use of out_count_host did not leave there */
    uint32_t reserved;
} tc_key_route;
/* r points at a tc_key_route (declared void* for the reason tc_throttle_batch_* give above) */
int tc_route_keys(tc_engine* e, const void* r);

/* ---- live state out of an engine, and into another --------------------------------------------------------------------------
 * A snapshot moves a whole engine into one of the same capacity and flags.  These two calls move ENTRIES: the live keys of an
 * engine (or of a page of its slots, or of the share one GPU of a new `world` will own) come out as the project's own arena form
 * with their TAT and expiry beside them, and such an arena is merged into any other engine -- a larger one (grow), the owner under
 * a new world (reshard: export with world / only, or export everything and split with tc_route_keys), a standby, or one that
 * already holds some of the keys (merge).  Device pointers throughout.
 * Engines: key-mode engines export and import keys, TAT and expiry; slot-mode engines (16-byte cells) the slot instead of the key.
 * TC_CFG_FIXED_PARAMS engines are OUT OF SCOPE: both calls return TC_E_UNSUPPORTED on them.  NOT CARRIED: denial counters
 * (TC_CFG_TRACK_DENIED) and the retired keys' counts stay where they are, and so do rate plans registered per slot.
 *
 * tc_export_live -- read-only, asynchronous on `stream`.  An entry is live iff expiry > now_ns (the reference's strict test,
 *   adaptive_cleanup.rs:248) and, in key mode, its slot is bound.  Entry k is the k-th live slot of the page, in ASCENDING slot order:
 *   out_slot[k], out_tat[k], out_expiry[k], and in key mode its key at out_key_bytes[out_key_off[k] .. out_key_off[k + 1]) -- the first
 *   offset is 0, the one behind the last entry is the byte total, so (out_key_bytes, out_key_off, count) is a complete arena for
 *   tc_route_keys, tc_rate_limit_batch_keys, tc_peek_batch_keys and tc_import_live.
 *   world >= 2 (key mode): only the keys whose owner under tc_route_keys_host's map is `only` -- from the hash the table stores, the
 *   key bytes are not hashed again.  world 0 or 1: every live key, `only` is ignored.
 *   out_count[0] = live entries of the page (after the owner filter), out_count[1] = their key bytes: always written.  If they exceed
 *   cap_entries or cap_bytes (or 2^32 - 1 bytes) NOTHING is written to the entry arrays: read the counts, come again with a smaller
 *   page or more room.  Nothing beyond the layout above is ever written (out_key_off takes cap_entries + 1 words).
 *   out_count_host: NULL, or three words of PINNED host memory (tc_host_alloc) that receive the two counts and then `tag`, as soon as
 *   the counts are known -- a caller that polls the tag learns how much room a repeat needs without a stream synchronisation; the
 *   entry arrays are complete when `stream` gets there.
 *   NOTHING CHANGES in the engine, as for tc_peek_batch_*: no cell, key-table word, counter, hint or sweep accounting.  Ordering: the
 *   export sees every call that returned before it and nothing of those after it -- on the engine's stream, behind the last key stage,
 *   and the key stage, sweep or rebuild of a later call waits for it; on a `stream` of the caller's the engine's stream is ordered
 *   in front of the export and behind it.  One export at a time is in flight (they share a scratch).
 *   Three launches, none of which waits for another workgroup.  struct_size too small, flags != 0, a page that is empty or reaches
 *   past the capacity, world > 64, world >= 2 with only outside [0, world) or on a slot-mode engine, a required array NULL (always
 *   out_tat, out_expiry, out_count; key mode out_key_bytes and out_key_off; slot mode out_slot): TC_E_INVALID_ARG, nothing is enqueued. */
typedef struct tc_export {
    uint32_t struct_size;     /* = sizeof(tc_export) */
    uint32_t flags;           /* must be 0 (flags to come are named TC_XP_*) */
    uint64_t first_slot;      /* the page: slots [first_slot, first_slot + n_slots) */
    uint64_t n_slots;
    int64_t now_ns;
    uint32_t world;           /* 0 / 1: every live key; 2..64 (key mode): the keys of destination `only` */
    int32_t only;
    uint64_t cap_entries;     /* room in the outputs: entries ... */
    uint64_t cap_bytes;       /* ... and key bytes */
    uint32_t* out_slot;       /* [cap_entries] source slot (slot mode: the key; key mode: optional, may be NULL) */
    uint8_t* out_key_bytes;   /* key mode: [cap_bytes] */
    uint32_t* out_key_off;    /* key mode: [cap_entries + 1] */
    int64_t* out_tat;         /* [cap_entries] */
    uint64_t* out_expiry;     /* [cap_entries] */
    uint64_t* out_count;      /* device [2] */
    uint64_t* out_count_host; /* NULL or pinned [3] */
    uint64_t tag;             /* any value the previous use of out_count_host did not leave there */
    void* stream;             /* NULL: the engine's stream */
} tc_export;
/* x points at a tc_export (declared void* for the reason tc_throttle_batch_* give above) */
int tc_export_live(tc_engine* e, const void* x);

/* tc_import_live -- merge n entries into the engine, on the engine's stream, ordered like any key work.
 *   Key mode: the arena is resolved by the insert stage of a key batch, unchanged (unknown keys are bound, duplicates inside the call
 *   share a slot, TC_CNT_KEYS_INSERTED and TC_CNT_LIVE_SLOTS move as for a batch).  Slot mode: slot[i] names the cell.
 *   The cell every entry of the call aimed at one slot leaves behind:
 *       expiry' = max(resident expiry, imported expiries)
 *       tat'    = max(imported tats, and the resident tat iff the resident expiry != 0)
 *   -- commutative and associative, so order and duplicates cannot matter; a larger TAT is more quota consumed, so the merged key is
 *   never more permissive than either source, and it stays resident as long as either would.  Exact for every int64 TAT.
 *   REJECTED (counted, nothing merged): an entry with expiry == 0 (it means vacant; in key mode its key is bound all the same, a bound
 *   slot with a vacant cell as a refused first request leaves one, which the next sweep frees), a slot >= capacity, a key that found
 *   no slot.  out_count[0] = entries merged, out_count[1] = entries rejected.
 *   Return: slot mode TC_E_OK, asynchronous.  Key mode: the call waits for its merge and reads the table's "full" word: TC_E_TABLE_FULL
 *   if a key found no slot (or that of an asynchronous batch before it did) -- the entries that fit were merged, as for
 *   tc_rate_limit_batch_keys.  Import does not run the cleanup policy, is not a batch (TC_CNT_BATCHES, TC_CNT_TOTAL), and leaves denial
 *   counters alone.  struct_size, flags != 0, n outside 1 .. max_batch, a required array NULL (always tat, expiry, out_count; key mode
 *   key_bytes and key_off; slot mode slot): TC_E_INVALID_ARG, nothing is enqueued. */
typedef struct tc_import {
    uint32_t struct_size;      /* = sizeof(tc_import) */
    uint32_t flags;            /* must be 0 */
    uint64_t n;                /* 1 .. max_batch */
    const uint32_t* slot;      /* slot mode: [n] */
    const uint8_t* key_bytes;  /* key mode: the arena ... */
    const uint32_t* key_off;   /* ... [n + 1] */
    const int64_t* tat;        /* [n] */
    const uint64_t* expiry;    /* [n] */
    uint64_t* out_count;       /* device [2] */
} tc_import;
/* m points at a tc_import */
int tc_import_live(tc_engine* e, const void* m);

/* tc_forget_batch -- remove n named keys (key mode) or slots (slot mode, wide or TC_CFG_FIXED_PARAMS) from the engine, whatever
 *   their expiry, on the engine's stream, ordered like any key work.  Device pointers throughout.  The reference has no such call: its
 *   map grows, and an entry leaves when it has expired and a cleanup runs.  Here a key that cannot be removed holds its slot until then.
 *   AFTER THE CALL every named key or slot behaves as if it had never been seen: the next request for it takes the reference's "first
 *   request" branch (rate_limiter.rs:162-166), a peek answers as for an unknown key, tc_export_live does not list it, and in key mode
 *   tc_lookup_slot returns -1.
 *   Key mode, every distinct key of the call that is bound: what a sweep does to a slot it unbinds -- the cell becomes {0, 0}, the slot
 *   is unbound and goes back onto the free stack (the next new key may take it), its denial count is retired to the key so that
 *   tc_top_denied_keys still reports it, the table entry becomes a tombstone (counted: the next sweep decides about a rebuild, as
 *   today), TC_CNT_LIVE_SLOTS drops by one.  An unknown key is not an error and changes nothing.  The overflow-arena bytes of a long
 *   key are reclaimed by the next sweep's compaction, as for swept keys.
 *   Slot mode: the cell becomes vacant ({0, 0}; TC_CFG_FIXED_PARAMS: the vacant TAT).  A slot >= capacity is ignored.  Denial counters
 *   stay (a slot is the key), and so do the plans registered per slot; on a TC_CFG_FIXED_PARAMS engine the call does not seal the
 *   plans, because it decides nothing.
 *   was_live[i] (if given) = 1 iff key or slot i held an entry with expiry > now_ns when the call began (the reference's strict test;
 *   fixed layout: expiry = TAT + the tolerance of the slot's registered plan), else 0.  Duplicates inside the call get identical
 *   answers, and the answer never depends on whether a sweep has run, as for peeks.  now_ns is used for nothing else: what is removed
 *   does not depend on it.
 *   out_count[0] = distinct entries removed (bound keys unbound, or non-vacant cells vacated), out_count[1] = how many of those were
 *   live at now_ns.
 *   NOT MOVED: TC_CNT_SWEPT, TC_CNT_BATCHES, TC_CNT_TOTAL, the cleanup policy's operation count (no sweep is triggered), grouping hints
 *   and the hot list, rate plans.
 *   Ordering: asynchronous, no host wait in either mode.  The call sees every call that returned before it (their evaluations are in
 *   front of it on the engine's stream; it goes behind the key stream's last stage), and the key stage, sweep or rebuild of any later
 *   call, pipelined ones included, waits for it.  Two launches, neither of which waits for another workgroup.
 *   struct_size too small, flags != 0, n outside 1 .. max_batch, out_count NULL, key mode with key_bytes or key_off NULL, slot mode
 *   with slot NULL: TC_E_INVALID_ARG, nothing is enqueued. */
typedef struct tc_forget {
    uint32_t struct_size;      /* = sizeof(tc_forget) */
    uint32_t flags;            /* must be 0 */
    uint64_t n;                /* 1 .. max_batch */
    const uint32_t* slot;      /* slot mode: [n] */
    const uint8_t* key_bytes;  /* key mode: the arena ... */
    const uint32_t* key_off;   /* ... [n + 1] */
    int64_t now_ns;            /* only for was_live / out_count[1]; what is removed does not depend on it */
    uint8_t* was_live;         /* [n] or NULL */
    uint64_t* out_count;       /* device [2], required */
} tc_forget;
/* f points at a tc_forget */
int tc_forget_batch(tc_engine* e, const void* f);

/* ---- pipeline health --------------------------------------------------------------------------------------------------------
 * Pipelined batches (TC_B_INPUTS_READY, TC_B_ASYNC, pinned host batches in chunks) are fast because their grouping runs on
 * internal streams BESIDE the evaluation of earlier batches.  Which hardware queue and dispatch pipe a stream lands on depends on
 * everything the process did with the GPU before, so the engine probes candidates against its main stream
 * and keeps those that really run concurrently -- and when it finds none (GPU_MAX_HW_QUEUES too small, a process full of streams)
 * the batches still give the same results, in order on the main stream, 1.5-2.5 x slower, without any error.  This call says
 * which of the two it is. */
typedef struct tc_engine_info {
    uint32_t struct_size;          /* = sizeof(tc_engine_info), set by the caller */
    uint32_t side_streams_probed;  /* 0: no pipelined batch yet on the current main stream -- nothing below is known */
    uint32_t grouping_streams_wanted;
    uint32_t grouping_streams;     /* kept after the probe; 0: pipelined batches run in order on the main stream */
    uint32_t key_stream;           /* string mode: 1 if key stages have a stream of their own */
    uint32_t candidates_tried;     /* streams created and probed */
    uint32_t rejected_same_queue;  /* ... that did not run while the main stream (or a kept stream) was running */
    uint32_t rejected_same_pipe;   /* ... that ran, but were handed out behind the main stream's workgroups */
    uint32_t kept_second_best;     /* kept although they share a dispatch pipe with ANOTHER kept stream (never with the main one) */
    uint32_t probes_assumed;       /* 1: TCGPU_ASSUME_CONCURRENT -- candidates taken unprobed (profiler counter passes) */
    uint32_t pipelining_degraded;  /* 1: fewer grouping streams than wanted (or no key stream): expect the slower figures */
    uint32_t scratch_sets;         /* batches whose grouping may be in flight at once */
    uint32_t grouping_path;        /* of the last batch: 0 none yet, 1 range path (2 launches), 2 LSD passes, 3 bucket path, 4 small batch / unique,
                                    * 5 range path with the hot slots peeled out (3 launches; skewed streams, round 6) */
    uint32_t range_path_possible;  /* the key space admits the range path */
    uint64_t range_hint_requests;  /* the range hint the next batch goes by: requests of the batch it came from ... */
    uint64_t range_hint_largest;   /* ... and its largest key range (a block finishes up to 4 096 requests in LDS) */
    uint64_t host_chunk_requests;  /* pinned synchronous host batches of at least twice this many requests are pipelined in chunks; 0: never */
    uint64_t batches;              /* batches decided so far */
    uint64_t hot_slots;            /* slots on the hot list right now (made from the evaluations' notes on long runs; 0: none) */
    uint64_t hot_batches;          /* batches grouped with the hot slots peeled out so far */
    uint64_t probes_pooled;        /* 1: the grouping streams came from the process's pool -- streams an earlier engine on this main stream
                                    * had probed, re-checked against the main stream instead of probing sixteen new candidates */
    uint64_t sweeps_aside;         /* string mode, round 6: explicit sweeps (tc_sweep_expired right behind a pipelined key batch) that ran on
                                    * the key stream BESIDE that batch's evaluation instead of behind it (TCGPU_SWEEP_ASIDE=0: never).  A caller
                                    * built against the struct without this field passes its smaller struct_size and gets the fields it knows */
} tc_engine_info;
int tc_engine_info_get(tc_engine* e, tc_engine_info* out);

/* Number of internal invariant violations the kernels have flagged since creation (always 0
 * unless there is a bug; the parity tests assert it). */
int tc_selfcheck(tc_engine* e, uint64_t* violations);

/* Test hook (error paths): the nth host <-> device staging copy from now fails with TC_E_HIP instead of being
 * issued; 0 disarms.  Not for production use. */
int tc_debug_fail_copy(tc_engine* e, uint32_t nth);
/* Test hook (watchdog): the next uniform batch's evaluation withholds the "row 0 has read its cells" announcement,
 * so a key whose requests span more than one row makes its owner wait until the watchdog gives up (2 s) and the
 * engine is poisoned (TC_E_INVARIANT).  Not for production use. */
int tc_debug_break_wait(tc_engine* e, uint32_t on);

/* Test hook (forward progress): a FILLER kernel -- `blocks` workgroups of 256 threads, `lds_bytes` of LDS each, every one of
 * which stays resident for `microseconds` -- enqueued on a stream of its own that is restricted to the compute units of
 * cu_mask (8 words, bit i = CU i as hipExtStreamCreateWithCUMask counts them; NULL: every CU).  Returns at once.  The
 * kernels that wait for other workgroups (radix look-back, direct stores, the general path's chain, the one-pass router)
 * wait only for workgroups dispatched EARLIER, so taking wave slots, LDS or whole CUs away from them must only ever make them
 * slower: tests/test_gpu_robustness.py runs them against fillers and checks results and watchdog.  Not for production use. */
int tc_debug_occupy(tc_engine* e, const uint32_t* cu_mask, uint32_t blocks, uint32_t lds_bytes, uint64_t microseconds);
/* Test hook (string keys): walks the key table both ways after draining the engine -- every bound slot must be reachable
 * through the entry its position column names (the entry binds that slot and carries the hash of the slot's key record),
 * every binding entry must name a bound slot that points back at it, no claim may be left pending, and bound slots + free
 * slots must add up to the capacity.  *inconsistencies = how many of these fail (0 on a
 * healthy table).  TC_E_UNSUPPORTED without TC_CFG_KEY_MODE.  Not for production use (two passes over the table). */
int tc_debug_check_keys(tc_engine* e, uint64_t* inconsistencies);

/* Checkpoint / restore of everything resident (state cells, rate plans, denial counters, in
 * string mode the key table, plus the counter block).  The reference keeps its state in memory
 * only and loses it on restart; here a snapshot is a few device-to-host copies.  Load needs an
 * engine created with the same capacity and flags.  Both calls drain the engine first. */
int tc_snapshot_save(tc_engine* e, const char* path);
int tc_snapshot_load(tc_engine* e, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* TCGPU_H */
