/* N-API addon over libbgv.so: the binding a Lodestar maintainer adds beside
 * chain/bls/multithread.  Plain C against
 * node_api.h (N-API v4+, Node >= 12), no node-addon-api / C++ wrapper.
 *
 *   abiVersion() -> number                      bgv_abi_version
 *   buildId() -> string                         bgv_build_id
 *   codeName(code) -> "BLST_..."                 bgv_set_code_name
 *   open(device, cuSplit = 0, cfg?) -> ctx (external)  bgv_open_cfg  (multithread/index.ts:120); cuSplit N > 0:
 *                                                a priority context on N reserved CUs (verifyOnMainThread),
 *                                                N < 0: a bulk context that leaves them free (bgv_cfg.cu_split);
 *                                                cfg (tests and A/B tools): {split, miller, hashDedup, millerSteps} as in bgv_cfg
 *   close(ctx)                                   bgv_close     (multithread/index.ts:193-214)
 *   pubkeysSet(ctx, first, Uint8Array, format)   bgv_pubkeys_set (pubkeyCache.ts:56-77)
 *   pubkeysCount(ctx) -> number
 *   pubkeysValidate(ctx, Uint8Array) -> Int32Array   bgv_pubkeys_validate (processDeposit.ts:57-66)
 *   verify(ctx, batch) -> Promise<result>        bgv_verify on the libuv pool (worker.ts:30-106)
 *   verifySync(ctx, batch) -> result             BlsSingleThreadVerifier (blocks the calling thread)
 *   partial(ctx, batch) -> Promise<result + {miller: Uint8Array(576), ok}>
 *                                                bgv_partial: one shard of a multi-GPU batch
 *   combineFinal(ctx, Uint8Array(576 n)) -> Promise<boolean>
 *                                                bgv_combine_final: ONE final exponentiation of the shards
 *   partialFinish(ctx) -> Promise<result>        bgv_partial_finish: localise the last partial()'s shard
 *                                                after a failed combined check
 *   verifySameMessage(ctx, smBatch) -> Promise<smResult>, verifySameMessageSync(ctx, smBatch) -> smResult
 *                                                bgv_verify_same_message (see "same-message batches" below)
 *   verifySameMessageAggregate(ctx, smBatch + {take?, prevSigs?}) -> Promise<smResult + {aggSigs, aggCount, aggCode}>,
 *   verifySameMessageAggregateSync(...)   bgv_verify_same_message_aggregate: the verdicts plus every group's aggregate signature
 *   verifySameMessageAgg(ctx, smaBatch) -> Promise<smResult>, verifySameMessageAggSync(ctx, smaBatch) -> smResult
 *   verifySameMessageBits(ctx, smbBatch) -> Promise<smResult>, verifySameMessageBitsSync(ctx, smbBatch) -> smResult
 *                                                bgv_verify_same_message_agg: the sets' keys are aggregates
 *   setIndexList(ctx, id, Uint32Array)           bgv_index_list_set: a resident index list (an epoch's shuffling,
 *                                                a sync committee); an empty array drops it
 *   indexListLen(ctx, id) -> number              bgv_index_list_len
 *   setIndexListSums(ctx, id, bool)              bgv_index_list_sums: build (or drop) the list's resident prefix sums
 *   indexListHasSums(ctx, id) -> boolean         bgv_index_list_has_sums
 *   hashStats(ctx) -> {sets, hashes, dedup}      bgv_hash_stats (the last verify / verifyBits / partial, for the sync paths)
 *   pairMerge(ctx, on)                           bgv_pair_merge: one Miller pair per distinct signing root of a job, from the
 *                                                next call on (bulk layout, one-lane loop; off by default)
 *   pairStats(ctx) -> {sets, pairs, merged, fallback}   bgv_pair_stats (the last verify / verifyBits / partial)
 *   smRetry(ctx, mode)                            bgv_sm_retry: the retry of the same-message entries, from the next call on:
 *                                                 0 one-set jobs (the default), 1 subs of 8, then the sets of the failing subs
 *   smRetryStats(ctx) -> {mode, segments, subs, subsFailed, leaves, pairs, hashes}   bgv_sm_retry_stats (the last same-message call)
 *   bitsPathStats(ctx) -> {setsComplement, keysExpanded, keysGathered}   bgv_bits_path_stats (the last verifyBits / verifySameMessageBits)
 *   verifyBits(ctx, bitsBatch) -> Promise<result>, verifyBitsSync(ctx, bitsBatch) -> result
 *                                                bgv_verify_bits: sets given as (list, window, participation bits)
 *                                                or as explicit index runs (see "committee bitfields" below)
 *
 * batch = {jobOffsets: Uint32Array, pkOffsets: Uint32Array, pkIndices:
 * Uint32Array, msgs: Uint8Array, sigs: Uint8Array (192 B per set), sigLen:
 * Uint32Array, rawPks?: Uint8Array (96 B per key)}.
 * result = {results: Int32Array (bgv_job_result per job: 1 valid, 0 invalid,
 * -code rejected), batchRetries, batchSigsSuccess, pubkeysAggregated,
 * deviceMs, workerStartMs, workerEndMs}: the BlsWorkResult fields
 * (multithread/types.ts:26-38) the pool's metrics are fed from; verify,
 * verifyBits and partial add hashes, the call's hash_to_G2 evaluations
 * (bgv_hash_stats, read while the context is still locked), and millerPairs,
 * the set pairs its Miller stage ran (bgv_pair_stats.pairs).  For
 * partial() `results` is provisional: -code for a job rejected by a parse /
 * subgroup / pubkey error (final), 1 for every other job (valid iff the
 * combined check passes).  Contexts on different devices run their queued
 * work concurrently on the libuv pool (one pool thread per call in flight:
 * size UV_THREADPOOL_SIZE >= the device count, napi/index.js does).
 *
 * Ownership: the offset arrays are copied when the call
 * is made and every length is checked against the copies, so a caller that
 * mutates its typed arrays while the work is queued cannot make the library
 * read past them; the other arrays are pinned by references until the work
 * completes (the library copies them to pinned memory and HBM and keeps
 * nothing).  The context external is referenced by every queued work item,
 * so it outlives them.  A context is not thread-safe: calls on one context
 * are serialised by its mutex. */
#include <node_api.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "bgv.h"

#define NAPI_CALL(env, call)                                              \
  do {                                                                    \
    if ((call) != napi_ok) {                                              \
      napi_throw_error((env), NULL, "bgv addon: N-API call failed: " #call); \
      return NULL;                                                        \
    }                                                                     \
  } while (0)

typedef struct {
  bgv_ctx* ctx;
  pthread_mutex_t mu;
  int closed;
  uint32_t partial_jobs; /* job count of the last partial() (sizes partialFinish's results) */
} addon_ctx;

static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  addon_ctx* c = (addon_ctx*)data;
  pthread_mutex_lock(&c->mu); /* no work item can hold the context here (each references it), but be exact */
  if (!c->closed) bgv_close(c->ctx);
  c->closed = 1;
  pthread_mutex_unlock(&c->mu);
  pthread_mutex_destroy(&c->mu);
  free(c);
}

static napi_value throw_bgv(napi_env env, int status) {
  char msg[512];
  snprintf(msg, sizeof msg, "bgv error %d: %s", status, bgv_last_error());
  napi_throw_error(env, NULL, msg);
  return NULL;
}

static addon_ctx* get_ctx(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "expected a bgv context");
    return NULL;
  }
  addon_ctx* c = (addon_ctx*)p;
  if (c->closed) {
    napi_throw_error(env, "QUEUE_ERROR_QUEUE_ABORTED", "QUEUE_ERROR_QUEUE_ABORTED: bgv context closed");
    return NULL;
  }
  return c;
}

/* the prologue of every (ctx, ...) entry: up to *argc arguments into a[], and the open context of a[0] */
static addon_ctx* ctx_args(napi_env env, napi_callback_info info, size_t* argc, napi_value* a) {
  if (napi_get_cb_info(env, info, argc, a, NULL, NULL) != napi_ok) {
    napi_throw_error(env, NULL, "bgv addon: N-API call failed: napi_get_cb_info(env, info, &argc, a, NULL, NULL)");
    return NULL;
  }
  return get_ctx(env, a[0]);
}
#define CTX_ARGS(n)                                  \
  size_t argc = (n);                                 \
  napi_value a[n];                                   \
  addon_ctx* c = ctx_args(env, info, &argc, a);      \
  if (!c) return NULL

/* one library call under the context's mutex (it waits for the context's batch in flight) */
#define LOCKED(c, st, call)           \
  do {                                \
    pthread_mutex_lock(&(c)->mu);     \
    (st) = (call);                    \
    pthread_mutex_unlock(&(c)->mu);   \
  } while (0)

/* typed-array view: data pointer and element count; -1 on type error */
static int typed(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len) {
  bool is = false;
  if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return -1;
  napi_typedarray_type t;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, v, &t, len, data, &ab, &off) != napi_ok || t != want) return -1;
  return 0;
}

/* a typed array of n elements of `elem` bytes over a copy of src */
static napi_value new_typed_array(napi_env env, napi_typedarray_type t, size_t elem, const void* src, size_t n) {
  void* dst = NULL;
  napi_value ab, arr;
  NAPI_CALL(env, napi_create_arraybuffer(env, elem * n, &dst, &ab));
  if (n) memcpy(dst, src, elem * n);
  NAPI_CALL(env, napi_create_typedarray(env, t, n, ab, 0, &arr));
  return arr;
}

/* sets o's named uint32 properties (o == NULL: on a new object); NULL after a throw */
typedef struct {
  const char* name;
  uint32_t val;
} named_u32;

static napi_value set_u32s(napi_env env, napi_value o, const named_u32* u, size_t n) {
  napi_value v;
  if (!o) NAPI_CALL(env, napi_create_object(env, &o));
  for (size_t k = 0; k < n; k++) {
    NAPI_CALL(env, napi_create_uint32(env, u[k].val, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, u[k].name, v));
  }
  return o;
}
#define SET_U32S(env, o, ...) set_u32s(env, o, (const named_u32[]){__VA_ARGS__}, sizeof((const named_u32[]){__VA_ARGS__}) / sizeof(named_u32))

static void set_double(napi_env env, napi_value o, const char* name, double x) {
  napi_value v;
  napi_create_double(env, x, &v);
  napi_set_named_property(env, o, name, v);
}

/* ------------------------------------------------------------------ sync */
static napi_value AbiVersion(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  NAPI_CALL(env, napi_create_int32(env, bgv_abi_version(), &r));
  return r;
}

static napi_value BuildId(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  NAPI_CALL(env, napi_create_string_utf8(env, bgv_build_id(), NAPI_AUTO_LENGTH, &r));
  return r;
}

static napi_value CodeName(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  int32_t code = 0;
  NAPI_CALL(env, napi_get_value_int32(env, a[0], &code));
  napi_value r;
  NAPI_CALL(env, napi_create_string_utf8(env, bgv_set_code_name(code), NAPI_AUTO_LENGTH, &r));
  return r;
}

static napi_value Open(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value a[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  int32_t dev = 0, cu_split = 0;
  if (argc >= 1) NAPI_CALL(env, napi_get_value_int32(env, a[0], &dev));
  if (argc >= 2) NAPI_CALL(env, napi_get_value_int32(env, a[1], &cu_split));
  bgv_cfg cfg;
  bgv_cfg_default(&cfg);
  cfg.cu_split = cu_split;
  if (argc >= 3) { /* pipeline overrides (tests, A/B tools): any other key is refused */
    napi_valuetype t;
    NAPI_CALL(env, napi_typeof(env, a[2], &t));
    if (t == napi_object) {
      napi_value keys, key, val;
      uint32_t nk = 0;
      NAPI_CALL(env, napi_get_property_names(env, a[2], &keys));
      NAPI_CALL(env, napi_get_array_length(env, keys, &nk));
      for (uint32_t k = 0; k < nk; k++) {
        char name[32];
        size_t len = 0;
        int32_t x = 0;
        NAPI_CALL(env, napi_get_element(env, keys, k, &key));
        NAPI_CALL(env, napi_get_value_string_utf8(env, key, name, sizeof name, &len));
        NAPI_CALL(env, napi_get_property(env, a[2], key, &val));
        NAPI_CALL(env, napi_get_value_int32(env, val, &x));
        if (!strcmp(name, "split")) cfg.split = x;
        else if (!strcmp(name, "miller")) cfg.miller = x;
        else if (!strcmp(name, "hashDedup")) cfg.hash_dedup = x;
        else if (!strcmp(name, "millerSteps")) cfg.miller_steps = x;
        else {
          napi_throw_type_error(env, NULL, "open: cfg takes split, miller, hashDedup and millerSteps");
          return NULL;
        }
      }
    } else if (t != napi_undefined && t != napi_null) {
      napi_throw_type_error(env, NULL, "open: cfg must be an object");
      return NULL;
    }
  }
  addon_ctx* c = (addon_ctx*)calloc(1, sizeof *c);
  if (!c) {
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  const int st = bgv_open_cfg(dev, &cfg, &c->ctx);
  if (st != BGV_OK) {
    free(c);
    return throw_bgv(env, st);
  }
  pthread_mutex_init(&c->mu, NULL);
  napi_value r;
  NAPI_CALL(env, napi_create_external(env, c, ctx_finalize, NULL, &r));
  return r;
}

static napi_value Close(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  pthread_mutex_lock(&c->mu);  /* waits for in-flight work */
  c->closed = 1;
  bgv_close(c->ctx);
  pthread_mutex_unlock(&c->mu);
  return NULL;
}

static napi_value PubkeysSet(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  uint32_t first = 0, fmt = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, a[1], &first));
  NAPI_CALL(env, napi_get_value_uint32(env, a[3], &fmt));
  void* data;
  size_t len;
  if (typed(env, a[2], napi_uint8_array, &data, &len)) {
    napi_throw_type_error(env, NULL, "pubkeys must be a Uint8Array");
    return NULL;
  }
  const size_t w = fmt == BGV_PK_UNCOMPRESSED_96 ? 96 : 48;
  int st;
  LOCKED(c, st, bgv_pubkeys_set(c->ctx, first, (uint32_t)(len / w), (const uint8_t*)data, fmt));
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

static napi_value PubkeysCount(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t n = 0;
  int st;
  LOCKED(c, st, bgv_pubkeys_count(c->ctx, &n));
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r;
  NAPI_CALL(env, napi_create_uint32(env, n, &r));
  return r;
}

static napi_value PubkeysValidate(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* data;
  size_t len;
  if (typed(env, a[1], napi_uint8_array, &data, &len)) {
    napi_throw_type_error(env, NULL, "pubkeys must be a Uint8Array of 48-byte keys");
    return NULL;
  }
  const uint32_t n = (uint32_t)(len / 48);
  int32_t* codes = (int32_t*)calloc(n ? n : 1, 4);
  if (!codes) {
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  int st;
  LOCKED(c, st, bgv_pubkeys_validate(c->ctx, (const uint8_t*)data, n, codes));
  napi_value r = st == BGV_OK ? new_typed_array(env, napi_int32_array, 4, codes, n) : throw_bgv(env, st);
  free(codes);
  return r;
}

/* ------------------------------------------------------------ batch fields
 * Every typed array a batch object can carry, whichever entry reads it: its name, its element type, whether a
 * batch may leave it out (FIELD_OPTIONAL: absent; FIELD_NULLABLE: absent, null or undefined), and whether it is
 * copied when the call is made (the offsets and the sources: every length is checked against the copy) or pinned
 * by a reference until the work completes.  An entry kind names its fields by a list of these rows. */
enum { F_JOB, F_GRP, F_PKO, F_SRC, F_BITS, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, F_TAKE, F_PREV, N_FIELDS, F_END = N_FIELDS };
enum { FIELD_REQUIRED, FIELD_OPTIONAL, FIELD_NULLABLE };
static const struct {
  const char* name;
  napi_typedarray_type type;
  size_t elem;
  int need;
  int copied;
} FIELD[N_FIELDS] = {
    [F_JOB] = {"jobOffsets", napi_uint32_array, 4, FIELD_REQUIRED, 1},
    [F_GRP] = {"groupOffsets", napi_uint32_array, 4, FIELD_REQUIRED, 1},
    [F_PKO] = {"pkOffsets", napi_uint32_array, 4, FIELD_REQUIRED, 1},
    [F_SRC] = {"src", napi_uint32_array, 4, FIELD_REQUIRED, 1},
    [F_BITS] = {"bits", napi_uint8_array, 1, FIELD_REQUIRED, 0},
    [F_PKI] = {"pkIndices", napi_uint32_array, 4, FIELD_REQUIRED, 0},
    [F_MSG] = {"msgs", napi_uint8_array, 1, FIELD_REQUIRED, 0},
    [F_SIG] = {"sigs", napi_uint8_array, 1, FIELD_REQUIRED, 0},
    [F_LEN] = {"sigLen", napi_uint32_array, 4, FIELD_REQUIRED, 0},
    [F_RAW] = {"rawPks", napi_uint8_array, 1, FIELD_OPTIONAL, 0},
    [F_TAKE] = {"take", napi_uint8_array, 1, FIELD_NULLABLE, 0},
    [F_PREV] = {"prevSigs", napi_uint8_array, 1, FIELD_NULLABLE, 0},
};
static const uint8_t VERIFY_FIELDS[] = {F_JOB, F_PKO, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, F_END};
static const uint8_t BITS_FIELDS[] = {F_JOB, F_SRC, F_BITS, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, F_END};
static const uint8_t SM_FIELDS[] = {F_GRP, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, F_END};
static const uint8_t SMA_FIELDS[] = {F_GRP, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, F_PKO, F_END};
static const uint8_t SMB_FIELDS[] = {F_GRP, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, F_SRC, F_BITS, F_END};
static const uint8_t TAKE_FIELD[] = {F_TAKE, F_END}, PREV_FIELD[] = {F_PREV, F_END};

/* ------------------------------------------------------------------- jobs
 * One job struct for every entry that runs a device call, on the libuv pool or on the calling thread. */
typedef enum {
  K_VERIFY,
  K_PARTIAL,
  K_BITS,
  K_FINISH,       /* partialFinish: no batch, results sized on the worker from the pending partial */
  K_COMBINE,      /* combineFinal: a copy of the partials, a boolean */
  K_SM,           /* verifySameMessage */
  K_SM_AGGREGATE, /* verifySameMessageAggregate: K_SM plus take / prevSigs and the groups' aggregates */
  K_SMA,          /* verifySameMessageAgg */
  K_SMB,          /* verifySameMessageBits */
  N_KINDS
} job_kind;
enum { O_JOBS, O_VALID, O_CODES, O_AGG_SIGS, O_AGG_COUNT, O_AGG_CODE, O_PARTS, N_OWNED };

typedef struct {
  addon_ctx* c;
  job_kind kind;
  void* ptr[N_FIELDS];    /* the batch's arrays: the copy of a copied field, else the caller's memory */
  size_t len[N_FIELDS];   /* element counts */
  void* copy[N_FIELDS];   /* copies made at call time (the library reads these) */
  napi_ref refs[N_FIELDS]; /* async: the pinned arrays */
  void* own[N_OWNED];     /* outputs (and K_COMBINE's copy of the partials), freed with the job */
  uint32_t n_jobs, n_sets, n_groups, n_parts;
  union {
    bgv_batch b;
    bgv_bits_batch bits;
    bgv_sm_batch sm;
    bgv_sma_batch sma;
    bgv_smb_batch smb;
  } u;
  bgv_sm_agg ag;          /* K_SM_AGGREGATE */
  uint8_t miller[576];    /* K_PARTIAL */
  int32_t ok;             /* K_PARTIAL: no job rejected; K_COMBINE: the product is 1 in GT */
  bgv_stats stats;
  bgv_sm_stats sm_stats;
  bgv_hash_path hash_path; /* K_VERIFY, K_BITS, K_PARTIAL: read under the context's lock */
  bgv_pair_path pair_path; /* likewise */
  bgv_bits_path bits_path; /* K_SMB: likewise */
  double t_start_ms, t_end_ms;
  int status;
  char err[512];
  napi_ref ctx_ref;
  napi_async_work work;
  napi_deferred deferred;
} job;

static int oom(napi_env env) {
  napi_throw_error(env, NULL, "out of memory");
  return -1;
}

static void job_free(napi_env env, job* j) {
  for (int k = 0; k < N_FIELDS; k++) {
    if (j->refs[k]) napi_delete_reference(env, j->refs[k]); /* unpin the inputs */
    free(j->copy[k]);
  }
  for (int k = 0; k < N_OWNED; k++) free(j->own[k]);
  if (j->ctx_ref) napi_delete_reference(env, j->ctx_ref);
}

/* zeroed output of n elements (at least one); -1 after throwing */
static int job_alloc(napi_env env, job* j, int slot, size_t n, size_t elem) {
  j->own[slot] = calloc(n ? n : 1, elem);
  return j->own[slot] ? 0 : oom(env);
}

/* the two refusals of a reader's own wording: a required field left out, a field of another type */
typedef struct {
  const char* missing;
  const char* wrong_type;
} field_refusals;
static const field_refusals BATCH_REFUSALS = {"batch field missing", "batch field has the wrong typed-array type"};
static const field_refusals BITS_REFUSALS = {"bits batch field missing", "bits batch field has the wrong typed-array type"};
static const field_refusals SUMS_REFUSALS = {NULL /* both rows are nullable */, "take / prevSigs must be a Uint8Array"};

/* THE reader: the listed fields of obj into j->ptr / j->len.  A field is looked up, type-checked, then copied or
 * (pin != 0) pinned; `say` words the refusals.  -1 after throwing. */
static int read_fields(napi_env env, napi_value obj, job* j, const uint8_t* fields, const field_refusals* say, int pin) {
  for (; *fields != F_END; fields++) {
    const int k = *fields;
    bool has = false;
    napi_value v;
    napi_has_named_property(env, obj, FIELD[k].name, &has);
    if (!has) {
      if (FIELD[k].need != FIELD_REQUIRED) continue;
      napi_throw_type_error(env, NULL, say->missing);
      return -1;
    }
    napi_get_named_property(env, obj, FIELD[k].name, &v);
    if (FIELD[k].need == FIELD_NULLABLE) {
      napi_valuetype vt;
      napi_typeof(env, v, &vt);
      if (vt == napi_undefined || vt == napi_null) continue;
    }
    if (typed(env, v, FIELD[k].type, &j->ptr[k], &j->len[k])) {
      napi_throw_type_error(env, NULL, say->wrong_type);
      j->ptr[k] = NULL;
      j->len[k] = 0;
      return -1;
    }
    if (FIELD[k].copied) {
      const size_t bytes = FIELD[k].elem * j->len[k];
      j->copy[k] = malloc(bytes ? bytes : 1);
      if (!j->copy[k]) return oom(env);
      if (bytes) memcpy(j->copy[k], j->ptr[k], bytes);
      j->ptr[k] = j->copy[k];
    } else if (pin) {
      napi_create_reference(env, v, 1, &j->refs[k]);
    }
  }
  return 0;
}

static int refuse_range(napi_env env, const char* msg) {
  napi_throw_range_error(env, NULL, msg);
  return -1;
}

/* what every bgv_*_batch holds per set, and what the two bitfield batches add; scalars stay NULL (drawn inside the
 * library: device ChaCha20 keyed by getrandom) and on_device 0 */
#define FILL_SETS(b, j)                                   \
  do {                                                    \
    (b).n_sets = (j)->n_sets;                             \
    (b).pk_indices = (const uint32_t*)(j)->ptr[F_PKI];    \
    (b).raw_pks = (const uint8_t*)(j)->ptr[F_RAW];        \
    (b).n_raw = (uint32_t)((j)->len[F_RAW] / 96);         \
    (b).msgs = (const uint8_t*)(j)->ptr[F_MSG];           \
    (b).sigs = (const uint8_t*)(j)->ptr[F_SIG];           \
    (b).sig_len = (const uint32_t*)(j)->ptr[F_LEN];       \
  } while (0)
#define FILL_SOURCES(b, j)                                \
  do {                                                    \
    FILL_SETS(b, j);                                      \
    (b).src = (const bgv_set_src*)(j)->ptr[F_SRC];        \
    (b).bits = (const uint8_t*)(j)->ptr[F_BITS];          \
    (b).bits_len = (uint32_t)(j)->len[F_BITS];            \
    (b).n_indices = (uint32_t)(j)->len[F_PKI];            \
  } while (0)

/* K_VERIFY, K_PARTIAL: batch = {jobOffsets, pkOffsets, pkIndices, msgs, sigs, sigLen, rawPks?} */
static int read_verify(napi_env env, napi_value obj, job* j, int pin) {
  const size_t* n = j->len;
  if (read_fields(env, obj, j, VERIFY_FIELDS, &BATCH_REFUSALS, pin)) return -1;
  if (n[F_JOB] < 1 || n[F_PKO] < 1) return refuse_range(env, "jobOffsets / pkOffsets need at least one entry");
  j->n_jobs = (uint32_t)(n[F_JOB] - 1);
  j->n_sets = (uint32_t)(n[F_PKO] - 1);
  if (n[F_MSG] < 32ull * j->n_sets || n[F_SIG] < 192ull * j->n_sets || n[F_LEN] < j->n_sets)
    return refuse_range(env, "msgs / sigs / sigLen shorter than the set count");
  if (n[F_PKI] < (size_t)((const uint32_t*)j->ptr[F_PKO])[j->n_sets]) return refuse_range(env, "pkIndices shorter than pkOffsets[n_sets]");
  FILL_SETS(j->u.b, j);
  j->u.b.n_jobs = j->n_jobs;
  j->u.b.job_offsets = (const uint32_t*)j->ptr[F_JOB];
  j->u.b.pk_offsets = (const uint32_t*)j->ptr[F_PKO];
  return job_alloc(env, j, O_JOBS, j->n_jobs, 4);
}

/* ------------------------------------------------------- committee bitfields
 * verifyBits(ctx, batch) -> Promise<result>, verifyBitsSync(ctx, batch) -> result (bgv_verify_bits).
 * batch = {jobOffsets: Uint32Array, src: Uint32Array (4 per set: list, off, len, bitsOff; list 0xffffffff = an
 * explicit run pkIndices[off .. off + len)), bits: Uint8Array (all bitfields, byte-packed, SSZ bit order),
 * pkIndices: Uint32Array (keys of the explicit sets), msgs, sigs, sigLen, rawPks? as for verify}.
 * result as for verify.  jobOffsets and src are copied at call time; the library stages every array into pinned
 * memory and checks the copy against the lengths taken here, so a caller that mutates its arrays while the work
 * is queued cannot make the device read past them. */
static int read_bits(napi_env env, napi_value obj, job* j, int pin) {
  const size_t* n = j->len;
  if (read_fields(env, obj, j, BITS_FIELDS, &BITS_REFUSALS, pin)) return -1;
  if (n[F_JOB] < 1 || n[F_SRC] % 4) return refuse_range(env, "jobOffsets needs at least one entry, src four entries per set");
  const size_t n_sets = n[F_SRC] / 4;
  if (n[F_MSG] < 32ull * n_sets || n[F_SIG] < 192ull * n_sets || n[F_LEN] < n_sets)
    return refuse_range(env, "msgs / sigs / sigLen shorter than the set count");
  if (n_sets > 0xffffffffull || n[F_BITS] > 0xffffffffull || n[F_PKI] > 0xffffffffull) return refuse_range(env, "bits batch too large");
  j->n_jobs = (uint32_t)(n[F_JOB] - 1);
  j->n_sets = (uint32_t)n_sets;
  FILL_SOURCES(j->u.bits, j);
  j->u.bits.n_jobs = j->n_jobs;
  j->u.bits.job_offsets = (const uint32_t*)j->ptr[F_JOB];
  return job_alloc(env, j, O_JOBS, j->n_jobs, 4);
}

/* ------------------------------------------------------- same-message batches
 * verifySameMessage(ctx, batch) -> Promise<result>, verifySameMessageSync(ctx, batch) -> result
 * (bgv_verify_same_message; IBlsVerifier.verifySignatureSetsSameMessage).
 * batch = {groupOffsets: Uint32Array, pkIndices: Uint32Array (one per set), msgs: Uint8Array (32 B per GROUP),
 * sigs: Uint8Array (192 B per set), sigLen: Uint32Array, rawPks?: Uint8Array}.
 * result = {valid: Uint8Array (1 / 0 per set), codes: Int32Array (bgv_set_code of a rejected set), segments,
 * hashes, pairs, groupsRetried, setsRetried, deviceMs, workerStartMs, workerEndMs}.  Ownership as for verify:
 * the offsets are copied at call time and every length is checked against the copy.
 *
 * verifySameMessageAgg / verifySameMessageAggSync (bgv_verify_same_message_agg): the same, with
 * pkOffsets: Uint32Array (n_sets + 1 entries, copied too) and pkIndices holding pkOffsets[n_sets] keys.
 *
 * verifySameMessageAggregate / verifySameMessageAggregateSync (bgv_verify_same_message_aggregate): the batch of
 * verifySameMessage plus take?: Uint8Array (one per set, 0 keeps a valid set out of its group's aggregate) and
 * prevSigs?: Uint8Array (96 B per GROUP, the running aggregates, compressed); the result gains aggSigs: Uint8Array
 * (96 B per group), aggCount: Uint32Array and aggCode: Int32Array (bgv_sm_agg). */
static int alloc_set_outputs(napi_env env, job* j) {
  return job_alloc(env, j, O_VALID, j->n_sets, 1) || job_alloc(env, j, O_CODES, j->n_sets, 4) ? -1 : 0;
}

/* K_SM_AGGREGATE, after the batch of K_SM: take and prevSigs, one after the other, and the groups' outputs */
static int read_sums(napi_env env, napi_value obj, job* j, int pin) {
  const size_t need[2] = {j->n_sets, 96ull * j->n_groups};
  const uint8_t* row[2] = {TAKE_FIELD, PREV_FIELD};
  for (int k = 0; k < 2; k++) {
    if (read_fields(env, obj, j, row[k], &SUMS_REFUSALS, pin)) return -1;
    if (j->ptr[row[k][0]] && j->len[row[k][0]] < need[k]) return refuse_range(env, "take / prevSigs shorter than the set / group count");
  }
  if (job_alloc(env, j, O_AGG_SIGS, j->n_groups, 96) || job_alloc(env, j, O_AGG_COUNT, j->n_groups, 4) ||
      job_alloc(env, j, O_AGG_CODE, j->n_groups, 4))
    return -1;
  j->ag.take = (const uint8_t*)j->ptr[F_TAKE];
  j->ag.prev_sig96 = (const uint8_t*)j->ptr[F_PREV];
  j->ag.agg_sig96 = (uint8_t*)j->own[O_AGG_SIGS];
  j->ag.agg_count = (uint32_t*)j->own[O_AGG_COUNT];
  j->ag.agg_code = (int32_t*)j->own[O_AGG_CODE];
  return 0;
}

/* K_SM, K_SM_AGGREGATE, K_SMA: the set count is the last group offset; K_SMA's key count the last key offset */
static int read_sm(napi_env env, napi_value obj, job* j, int pin) {
  const size_t* n = j->len;
  if (read_fields(env, obj, j, j->kind == K_SMA ? SMA_FIELDS : SM_FIELDS, &BATCH_REFUSALS, pin)) return -1;
  if (n[F_GRP] < 1) return refuse_range(env, "groupOffsets needs at least one entry");
  j->n_groups = (uint32_t)(n[F_GRP] - 1);
  j->n_sets = ((const uint32_t*)j->ptr[F_GRP])[j->n_groups];
  size_t n_keys = j->n_sets;
  if (j->kind == K_SMA) {
    if (n[F_PKO] < (size_t)j->n_sets + 1) return refuse_range(env, "pkOffsets shorter than the set count + 1");
    n_keys = ((const uint32_t*)j->ptr[F_PKO])[j->n_sets];
  }
  if (n[F_MSG] < 32ull * j->n_groups || n[F_SIG] < 192ull * j->n_sets || n[F_LEN] < j->n_sets || n[F_PKI] < n_keys)
    return refuse_range(env, "msgs / sigs / sigLen / pkIndices shorter than the group, set or key count");
  if (alloc_set_outputs(env, j)) return -1;
  if (j->kind == K_SMA) {
    FILL_SETS(j->u.sma, j);
    j->u.sma.n_groups = j->n_groups;
    j->u.sma.group_offsets = (const uint32_t*)j->ptr[F_GRP];
    j->u.sma.pk_offsets = (const uint32_t*)j->ptr[F_PKO];
    return 0;
  }
  FILL_SETS(j->u.sm, j);
  j->u.sm.n_groups = j->n_groups;
  j->u.sm.group_offsets = (const uint32_t*)j->ptr[F_GRP];
  return j->kind == K_SM_AGGREGATE ? read_sums(env, obj, j, pin) : 0;
}

/* verifySameMessageBits(ctx, batch) -> Promise<result>, verifySameMessageBitsSync(ctx, batch) -> result
 * (bgv_verify_same_message_bits).  batch = {groupOffsets, src: Uint32Array (4 per set, as verifyBits), bits:
 * Uint8Array, pkIndices: Uint32Array (keys of the explicit sets), msgs (32 B per GROUP), sigs, sigLen, rawPks?}.
 * result as verifySameMessageAgg plus pubkeysAggregated, the participating keys from the call's path counters
 * (the caller holds no index lists to count them from).  Ownership as for verifyBits: groupOffsets and src are
 * copied at call time, the other typed arrays are pinned until completion. */
static int read_smb(napi_env env, napi_value obj, job* j, int pin) {
  const size_t* n = j->len;
  if (read_fields(env, obj, j, SMB_FIELDS, &BATCH_REFUSALS, pin)) return -1;
  if (n[F_GRP] < 1 || n[F_SRC] % 4) return refuse_range(env, "groupOffsets needs at least one entry, src four entries per set");
  const size_t n_sets = n[F_SRC] / 4;
  if (n_sets > 0xffffffffull || n[F_BITS] > 0xffffffffull || n[F_PKI] > 0xffffffffull) return refuse_range(env, "bits batch too large");
  j->n_groups = (uint32_t)(n[F_GRP] - 1);
  j->n_sets = (uint32_t)n_sets;
  if (((const uint32_t*)j->ptr[F_GRP])[j->n_groups] != n_sets) return refuse_range(env, "groupOffsets must end at the set count of src");
  if (n[F_MSG] < 32ull * j->n_groups || n[F_SIG] < 192ull * n_sets || n[F_LEN] < n_sets)
    return refuse_range(env, "msgs / sigs / sigLen shorter than the group or set count");
  FILL_SOURCES(j->u.smb, j);
  j->u.smb.n_groups = j->n_groups;
  j->u.smb.group_offsets = (const uint32_t*)j->ptr[F_GRP];
  return alloc_set_outputs(env, j);
}

/* ---------------------------------------------------------------- results */
/* the kinds whose hash and pair counters are read with the call and reported with its result */
static int counted(job_kind k) { return k == K_VERIFY || k == K_BITS || k == K_PARTIAL; }

/* deviceMs, workerStartMs, workerEndMs: what the pool's timing metrics are fed from */
static void set_times(napi_env env, napi_value o, const job* j, float device_ms) {
  set_double(env, o, "deviceMs", (double)device_ms);
  set_double(env, o, "workerStartMs", j->t_start_ms);
  set_double(env, o, "workerEndMs", j->t_end_ms);
}

static int set_array(napi_env env, napi_value o, const char* name, napi_typedarray_type t, size_t elem, const void* src, size_t n) {
  napi_value v = new_typed_array(env, t, elem, src, n);
  if (!v) return -1;
  napi_set_named_property(env, o, name, v);
  return 0;
}

/* {results, batchRetries, batchSigsSuccess, pubkeysAggregated, deviceMs, workerStartMs, workerEndMs}; verify, verifyBits
 * and partial add {hashes, millerPairs}, partial {miller, ok} */
static napi_value result_object(napi_env env, const job* j) {
  napi_value o, v;
  if (napi_create_object(env, &o) != napi_ok) return NULL;
  if (set_array(env, o, "results", napi_int32_array, 4, j->own[O_JOBS], j->n_jobs)) return NULL;
  if (!SET_U32S(env, o, {"batchRetries", j->stats.batch_retries}, {"batchSigsSuccess", j->stats.batch_sigs_success})) return NULL;
  set_double(env, o, "pubkeysAggregated", (double)j->stats.pubkeys_aggregated);
  set_times(env, o, j, j->stats.total_ms);
  if (counted(j->kind) && !SET_U32S(env, o, {"hashes", j->hash_path.hashes}, {"millerPairs", j->pair_path.pairs})) return NULL;
  if (j->kind == K_PARTIAL) {
    if (set_array(env, o, "miller", napi_uint8_array, 1, j->miller, 576)) return NULL;
    napi_get_boolean(env, j->ok != 0, &v);
    napi_set_named_property(env, o, "ok", v);
  }
  return o;
}

/* {valid, codes, segments, hashes, pairs, groupsRetried, setsRetried, deviceMs, workerStartMs, workerEndMs}; K_SMB adds
 * pubkeysAggregated, K_SM_AGGREGATE {aggSigs, aggCount, aggCode} */
static napi_value sm_result(napi_env env, const job* j) {
  napi_value o;
  const bgv_sm_stats* s = &j->sm_stats;
  if (napi_create_object(env, &o) != napi_ok) return NULL;
  if (set_array(env, o, "valid", napi_uint8_array, 1, j->own[O_VALID], j->n_sets) ||
      set_array(env, o, "codes", napi_int32_array, 4, j->own[O_CODES], j->n_sets))
    return NULL;
  if (!SET_U32S(env, o, {"segments", s->n_segments}, {"hashes", s->hashes}, {"pairs", s->pairs}, {"groupsRetried", s->groups_retried},
                {"setsRetried", s->sets_retried}))
    return NULL;
  if (j->kind == K_SMB && !SET_U32S(env, o, {"pubkeysAggregated", j->bits_path.keys_expanded})) return NULL;
  if (j->kind == K_SM_AGGREGATE) {
    const size_t G = j->n_sets ? j->n_groups : 0; /* an empty batch writes nothing */
    if (set_array(env, o, "aggSigs", napi_uint8_array, 1, j->own[O_AGG_SIGS], 96 * G) ||
        set_array(env, o, "aggCount", napi_uint32_array, 4, j->own[O_AGG_COUNT], G) ||
        set_array(env, o, "aggCode", napi_int32_array, 4, j->own[O_AGG_CODE], G))
      return NULL;
  }
  set_times(env, o, j, s->total_ms);
  return o;
}

static napi_value combine_result(napi_env env, const job* j) {
  napi_value b;
  napi_get_boolean(env, j->ok != 0, &b);
  return b;
}

/* per kind: the reader of its batch (none: the entry fills the job itself), the result it settles with, the label
 * of its async work and the arguments its entry takes */
static const struct {
  int (*read)(napi_env, napi_value, job*, int pin);
  napi_value (*result)(napi_env, const job*);
  const char* label;
  size_t arity;
} KIND[N_KINDS] = {
    [K_VERIFY] = {read_verify, result_object, "bgv_verify", 2},
    [K_PARTIAL] = {read_verify, result_object, "bgv_partial", 2},
    [K_BITS] = {read_bits, result_object, "bgv_verify_bits", 2},
    [K_FINISH] = {NULL, result_object, "bgv_partial_finish", 1},
    [K_COMBINE] = {NULL, combine_result, "bgv_combine_final", 2},
    [K_SM] = {read_sm, sm_result, "bgv_verify_same_message", 2},
    [K_SM_AGGREGATE] = {read_sm, sm_result, "bgv_verify_same_message_aggregate", 2},
    [K_SMA] = {read_sm, sm_result, "bgv_verify_same_message_agg", 2},
    [K_SMB] = {read_smb, sm_result, "bgv_verify_same_message_bits", 2},
};

/* ------------------------------------------------------------ running a job */
static double now_ms(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec * 1e3 + (double)t.tv_nsec * 1e-6;
}

static int job_call(job* j) {
  bgv_ctx* x = j->c->ctx;
  int st;
  switch (j->kind) {
    case K_VERIFY: return bgv_verify(x, &j->u.b, (int32_t*)j->own[O_JOBS], NULL, &j->stats);
    case K_BITS: return bgv_verify_bits(x, &j->u.bits, (int32_t*)j->own[O_JOBS], NULL, &j->stats);
    case K_PARTIAL:
      st = bgv_partial(x, &j->u.b, j->miller, NULL, (int32_t*)j->own[O_JOBS], &j->ok);
      j->c->partial_jobs = j->n_jobs;
      if (st != BGV_OK) return st;
      st = bgv_last_stats(x, &j->stats);
      j->stats.pubkeys_aggregated = j->n_sets ? j->u.b.pk_offsets[j->n_sets] : 0;
      return st;
    case K_FINISH:
      j->n_jobs = j->c->partial_jobs;
      j->own[O_JOBS] = calloc(j->n_jobs ? j->n_jobs : 1, 4);
      return j->own[O_JOBS] ? bgv_partial_finish(x, (int32_t*)j->own[O_JOBS], &j->stats) : BGV_E_INVALID_ARG;
    case K_COMBINE: return bgv_combine_final(x, (const uint8_t*)j->own[O_PARTS], j->n_parts, &j->ok);
    case K_SM: return bgv_verify_same_message(x, &j->u.sm, (uint8_t*)j->own[O_VALID], (int32_t*)j->own[O_CODES], &j->sm_stats);
    case K_SM_AGGREGATE:
      return bgv_verify_same_message_aggregate(x, &j->u.sm, &j->ag, (uint8_t*)j->own[O_VALID], (int32_t*)j->own[O_CODES], &j->sm_stats);
    case K_SMA: return bgv_verify_same_message_agg(x, &j->u.sma, (uint8_t*)j->own[O_VALID], (int32_t*)j->own[O_CODES], &j->sm_stats);
    case K_SMB:
      st = bgv_verify_same_message_bits(x, &j->u.smb, (uint8_t*)j->own[O_VALID], (int32_t*)j->own[O_CODES], &j->sm_stats);
      return st == BGV_OK ? bgv_bits_path_stats(x, &j->bits_path) : st; /* under the same lock: this call's */
    default: return BGV_E_INVALID_ARG;
  }
}

static void job_run(job* j) {
  pthread_mutex_lock(&j->c->mu);
  j->t_start_ms = now_ms();
  if (j->c->closed) {
    j->status = BGV_E_INVALID_ARG;
    snprintf(j->err, sizeof j->err, "QUEUE_ERROR_QUEUE_ABORTED");
  } else {
    j->status = job_call(j);
    /* under the same lock: this call's evaluations, not a later call's */
    if (j->status == BGV_OK && counted(j->kind)) j->status = bgv_hash_stats(j->c->ctx, &j->hash_path);
    if (j->status == BGV_OK && counted(j->kind)) j->status = bgv_pair_stats(j->c->ctx, &j->pair_path);
    if (j->status != BGV_OK) snprintf(j->err, sizeof j->err, "bgv error %d: %s", j->status, bgv_last_error());
  }
  j->t_end_ms = now_ms();
  pthread_mutex_unlock(&j->c->mu);
}

static void job_exec(napi_env env, void* data) { /* libuv worker thread */
  (void)env;
  job_run((job*)data);
}

static void job_done(napi_env env, napi_status st, void* data) { /* main thread */
  job* j = (job*)data;
  if (st != napi_ok && j->status == BGV_OK) {
    j->status = BGV_E_INVALID_ARG;
    snprintf(j->err, sizeof j->err, "async work cancelled");
  }
  if (j->status != BGV_OK) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->err, NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_resolve_deferred(env, j->deferred, KIND[j->kind].result(env, j));
  }
  napi_delete_async_work(env, j->work);
  job_free(env, j);
  free(j);
}

/* queues j on the libuv pool; the promise settles in job_done.  A job that cannot be queued is freed here. */
static napi_value job_queue(napi_env env, napi_value ctx_val, job* j) {
  napi_value promise, name;
  const char* failed = NULL;
  if (napi_create_reference(env, ctx_val, 1, &j->ctx_ref) != napi_ok) failed = "napi_create_reference"; /* the context outlives its queued work */
  else if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) failed = "napi_create_promise";
  else if (napi_create_string_utf8(env, KIND[j->kind].label, NAPI_AUTO_LENGTH, &name) != napi_ok) failed = "napi_create_string_utf8";
  else if (napi_create_async_work(env, NULL, name, job_exec, job_done, j, &j->work) != napi_ok) failed = "napi_create_async_work";
  else if (napi_queue_async_work(env, j->work) != napi_ok) failed = "napi_queue_async_work";
  if (!failed) return promise;
  char msg[96];
  snprintf(msg, sizeof msg, "bgv addon: N-API call failed: %s", failed);
  if (j->work) napi_delete_async_work(env, j->work);
  job_free(env, j);
  free(j);
  napi_throw_error(env, NULL, msg);
  return NULL;
}

/* runs j on the calling thread */
static napi_value job_sync(napi_env env, job* j) {
  job_run(j);
  if (j->status == BGV_OK) return KIND[j->kind].result(env, j);
  napi_throw_error(env, NULL, j->err);
  return NULL;
}

/* every entry that runs a device call: (ctx, batch) read by the kind's reader, then on the pool (the arrays that
 * are not copied pinned) or, sync, on this thread (nothing pinned: the call returns before the caller runs again) */
static napi_value job_entry(napi_env env, napi_callback_info info, job_kind kind, int sync) {
  size_t argc = KIND[kind].arity;
  napi_value a[2], r = NULL;
  addon_ctx* c = ctx_args(env, info, &argc, a);
  if (!c) return NULL;
  job* j = (job*)calloc(1, sizeof *j);
  if (!j) {
    oom(env);
    return NULL;
  }
  j->c = c;
  j->kind = kind;
  if (kind == K_COMBINE) {
    void* data;
    size_t len;
    if (argc < 2 || typed(env, a[1], napi_uint8_array, &data, &len) || len % 576) {
      napi_throw_type_error(env, NULL, "combineFinal(ctx, Uint8Array of 576-byte partials)");
    } else if (!(j->own[O_PARTS] = malloc(len ? len : 1))) { /* copied: the caller may reuse its buffer */
      oom(env);
    } else {
      if (len) memcpy(j->own[O_PARTS], data, len);
      j->n_parts = (uint32_t)(len / 576);
      return job_queue(env, a[0], j);
    }
  } else if (!KIND[kind].read || !KIND[kind].read(env, a[1], j, !sync)) {
    if (!sync) return job_queue(env, a[0], j);
    r = job_sync(env, j);
  }
  job_free(env, j);
  free(j);
  return r;
}

static napi_value Verify(napi_env env, napi_callback_info info) { return job_entry(env, info, K_VERIFY, 0); }
static napi_value VerifySync(napi_env env, napi_callback_info info) { return job_entry(env, info, K_VERIFY, 1); }
static napi_value Partial(napi_env env, napi_callback_info info) { return job_entry(env, info, K_PARTIAL, 0); }
/* partialFinish(ctx): the shard left by the last partial() on the context */
static napi_value PartialFinish(napi_env env, napi_callback_info info) { return job_entry(env, info, K_FINISH, 0); }
static napi_value CombineFinal(napi_env env, napi_callback_info info) { return job_entry(env, info, K_COMBINE, 0); }
static napi_value VerifyBits(napi_env env, napi_callback_info info) { return job_entry(env, info, K_BITS, 0); }
static napi_value VerifyBitsSync(napi_env env, napi_callback_info info) { return job_entry(env, info, K_BITS, 1); }
static napi_value VerifySameMessage(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SM, 0); }
static napi_value VerifySameMessageSync(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SM, 1); }
static napi_value VerifySameMessageAgg(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SMA, 0); }
static napi_value VerifySameMessageAggSync(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SMA, 1); }
static napi_value VerifySameMessageAggregate(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SM_AGGREGATE, 0); }
static napi_value VerifySameMessageAggregateSync(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SM_AGGREGATE, 1); }
static napi_value VerifySameMessageBits(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SMB, 0); }
static napi_value VerifySameMessageBitsSync(napi_env env, napi_callback_info info) { return job_entry(env, info, K_SMB, 1); }

/* ------------------------------------------------- index lists and counters */
static napi_value SetIndexList(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  uint32_t id = 0;
  void* data = NULL;
  size_t len = 0;
  if (argc < 3 || napi_get_value_uint32(env, a[1], &id) != napi_ok || typed(env, a[2], napi_uint32_array, &data, &len) ||
      len > 0xffffffffull) {
    napi_throw_type_error(env, NULL, "setIndexList(ctx, id, Uint32Array)");
    return NULL;
  }
  int st;
  LOCKED(c, st, bgv_index_list_set(c->ctx, id, (const uint32_t*)data, (uint32_t)len));
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

static napi_value IndexListLen(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  uint32_t id = 0, n = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, a[1], &id));
  int st;
  LOCKED(c, st, bgv_index_list_len(c->ctx, id, &n));
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r;
  NAPI_CALL(env, napi_create_uint32(env, n, &r));
  return r;
}

static napi_value SetIndexListSums(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  uint32_t id = 0;
  bool enable = false;
  if (argc < 3 || napi_get_value_uint32(env, a[1], &id) != napi_ok || napi_get_value_bool(env, a[2], &enable) != napi_ok) {
    napi_throw_type_error(env, NULL, "setIndexListSums(ctx, id, boolean)");
    return NULL;
  }
  int st;
  LOCKED(c, st, bgv_index_list_sums(c->ctx, id, enable ? 1u : 0u));
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

static napi_value IndexListHasSums(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  uint32_t id = 0, has = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, a[1], &id));
  int st;
  LOCKED(c, st, bgv_index_list_has_sums(c->ctx, id, &has));
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r;
  NAPI_CALL(env, napi_get_boolean(env, has != 0, &r));
  return r;
}

/* hashStats(ctx): bgv_hash_stats of the context's last ordinary batch (the sync paths read it after the call) */
static napi_value HashStats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  bgv_hash_path p;
  int st;
  LOCKED(c, st, bgv_hash_stats(c->ctx, &p));
  if (st != BGV_OK) return throw_bgv(env, st);
  return SET_U32S(env, NULL, {"sets", p.sets}, {"hashes", p.hashes}, {"dedup", p.dedup});
}

/* pairStats(ctx): bgv_pair_stats of the context's last ordinary batch */
static napi_value PairStats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  bgv_pair_path p;
  int st;
  LOCKED(c, st, bgv_pair_stats(c->ctx, &p));
  if (st != BGV_OK) return throw_bgv(env, st);
  return SET_U32S(env, NULL, {"sets", p.sets}, {"pairs", p.pairs}, {"merged", p.merged}, {"fallback", p.fallback});
}

/* smRetryStats(ctx): bgv_sm_retry_stats of the context's last same-message call */
static napi_value SmRetryStats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  bgv_sm_retry_path p;
  int st;
  LOCKED(c, st, bgv_sm_retry_stats(c->ctx, &p));
  if (st != BGV_OK) return throw_bgv(env, st);
  return SET_U32S(env, NULL, {"mode", p.mode}, {"segments", p.segments}, {"subs", p.subs}, {"subsFailed", p.subs_failed},
                  {"leaves", p.leaves}, {"pairs", p.pairs}, {"hashes", p.hashes});
}

static napi_value BitsPathStats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  bgv_bits_path p;
  int st;
  LOCKED(c, st, bgv_bits_path_stats(c->ctx, &p));
  if (st != BGV_OK) return throw_bgv(env, st);
  return SET_U32S(env, NULL, {"setsComplement", p.sets_complement}, {"keysExpanded", p.keys_expanded}, {"keysGathered", p.keys_gathered});
}

/* (ctx, mode) for a library switch: a boolean, or 0 / 1; any other number is refused by the library */
static napi_value set_mode(napi_env env, napi_callback_info info, int (*apply)(bgv_ctx*, int32_t)) {
  CTX_ARGS(2);
  int32_t mode = 0;
  napi_valuetype t = napi_undefined;
  if (argc >= 2) NAPI_CALL(env, napi_typeof(env, a[1], &t));
  if (t == napi_boolean) {
    bool on = false;
    NAPI_CALL(env, napi_get_value_bool(env, a[1], &on));
    mode = on ? 1 : 0;
  } else {
    NAPI_CALL(env, napi_get_value_int32(env, a[1], &mode));
  }
  int st;
  LOCKED(c, st, apply(c->ctx, mode));
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

/* pairMerge(ctx, on): bgv_pair_merge */
static napi_value PairMerge(napi_env env, napi_callback_info info) { return set_mode(env, info, bgv_pair_merge); }
/* smRetry(ctx, mode): bgv_sm_retry */
static napi_value SmRetry(napi_env env, napi_callback_info info) { return set_mode(env, info, bgv_sm_retry); }

static napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor d[] = {
      {"abiVersion", NULL, AbiVersion, NULL, NULL, NULL, napi_enumerable, NULL},
      {"buildId", NULL, BuildId, NULL, NULL, NULL, napi_enumerable, NULL},
      {"codeName", NULL, CodeName, NULL, NULL, NULL, napi_enumerable, NULL},
      {"open", NULL, Open, NULL, NULL, NULL, napi_enumerable, NULL},
      {"close", NULL, Close, NULL, NULL, NULL, napi_enumerable, NULL},
      {"pubkeysSet", NULL, PubkeysSet, NULL, NULL, NULL, napi_enumerable, NULL},
      {"pubkeysCount", NULL, PubkeysCount, NULL, NULL, NULL, napi_enumerable, NULL},
      {"pubkeysValidate", NULL, PubkeysValidate, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verify", NULL, Verify, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySync", NULL, VerifySync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"partial", NULL, Partial, NULL, NULL, NULL, napi_enumerable, NULL},
      {"partialFinish", NULL, PartialFinish, NULL, NULL, NULL, napi_enumerable, NULL},
      {"combineFinal", NULL, CombineFinal, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessage", NULL, VerifySameMessage, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageSync", NULL, VerifySameMessageSync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageAggregate", NULL, VerifySameMessageAggregate, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageAggregateSync", NULL, VerifySameMessageAggregateSync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageAgg", NULL, VerifySameMessageAgg, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageAggSync", NULL, VerifySameMessageAggSync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageBits", NULL, VerifySameMessageBits, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifySameMessageBitsSync", NULL, VerifySameMessageBitsSync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setIndexList", NULL, SetIndexList, NULL, NULL, NULL, napi_enumerable, NULL},
      {"indexListLen", NULL, IndexListLen, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setIndexListSums", NULL, SetIndexListSums, NULL, NULL, NULL, napi_enumerable, NULL},
      {"indexListHasSums", NULL, IndexListHasSums, NULL, NULL, NULL, napi_enumerable, NULL},
      {"bitsPathStats", NULL, BitsPathStats, NULL, NULL, NULL, napi_enumerable, NULL},
      {"hashStats", NULL, HashStats, NULL, NULL, NULL, napi_enumerable, NULL},
      {"pairMerge", NULL, PairMerge, NULL, NULL, NULL, napi_enumerable, NULL},
      {"pairStats", NULL, PairStats, NULL, NULL, NULL, napi_enumerable, NULL},
      {"smRetry", NULL, SmRetry, NULL, NULL, NULL, napi_enumerable, NULL},
      {"smRetryStats", NULL, SmRetryStats, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifyBits", NULL, VerifyBits, NULL, NULL, NULL, napi_enumerable, NULL},
      {"verifyBitsSync", NULL, VerifyBitsSync, NULL, NULL, NULL, napi_enumerable, NULL},
  };
  if (napi_define_properties(env, exports, sizeof d / sizeof d[0], d) != napi_ok) return NULL;
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
