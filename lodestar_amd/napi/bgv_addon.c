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
  bgv_ctx* ctx = NULL;
  const int st = bgv_open_cfg(dev, &cfg, &ctx);
  if (st != BGV_OK) return throw_bgv(env, st);
  addon_ctx* c = (addon_ctx*)calloc(1, sizeof *c);
  c->ctx = ctx;
  pthread_mutex_init(&c->mu, NULL);
  napi_value r;
  NAPI_CALL(env, napi_create_external(env, c, ctx_finalize, NULL, &r));
  return r;
}

static napi_value Close(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  pthread_mutex_lock(&c->mu);  /* waits for in-flight work */
  c->closed = 1;
  bgv_close(c->ctx);
  pthread_mutex_unlock(&c->mu);
  return NULL;
}

static napi_value PubkeysSet(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value a[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
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
  pthread_mutex_lock(&c->mu);
  const int st = bgv_pubkeys_set(c->ctx, first, (uint32_t)(len / w), (const uint8_t*)data, fmt);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

static napi_value PubkeysCount(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  uint32_t n = 0;
  pthread_mutex_lock(&c->mu);
  const int st = bgv_pubkeys_count(c->ctx, &n);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r;
  NAPI_CALL(env, napi_create_uint32(env, n, &r));
  return r;
}

static napi_value new_int32_array(napi_env env, const int32_t* src, size_t n) {
  void* dst = NULL;
  napi_value ab, arr;
  NAPI_CALL(env, napi_create_arraybuffer(env, 4 * n, &dst, &ab));
  if (n) memcpy(dst, src, 4 * n);
  NAPI_CALL(env, napi_create_typedarray(env, napi_int32_array, n, ab, 0, &arr));
  return arr;
}

static napi_value PubkeysValidate(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (typed(env, a[1], napi_uint8_array, &data, &len)) {
    napi_throw_type_error(env, NULL, "pubkeys must be a Uint8Array of 48-byte keys");
    return NULL;
  }
  const uint32_t n = (uint32_t)(len / 48);
  int32_t* codes = (int32_t*)calloc(n ? n : 1, 4);
  pthread_mutex_lock(&c->mu);
  const int st = bgv_pubkeys_validate(c->ctx, (const uint8_t*)data, n, codes);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) {
    free(codes);
    return throw_bgv(env, st);
  }
  napi_value r = new_int32_array(env, codes, n);
  free(codes);
  return r;
}

/* ----------------------------------------------------------------- verify */
enum { F_JOB, F_PKO, F_PKI, F_MSG, F_SIG, F_LEN, F_RAW, N_FIELDS };
static const char* FIELD[N_FIELDS] = {"jobOffsets", "pkOffsets", "pkIndices", "msgs", "sigs", "sigLen", "rawPks"};
static const napi_typedarray_type FIELD_T[N_FIELDS] = {napi_uint32_array, napi_uint32_array, napi_uint32_array,
                                                       napi_uint8_array,  napi_uint8_array,  napi_uint32_array,
                                                       napi_uint8_array};

enum { K_VERIFY, K_PARTIAL, K_FINISH, K_COMBINE, K_BITS };
/* bgv_bits_batch fields (K_BITS) */
enum { B_JOB, B_SRC, B_BITS, B_PKI, B_MSG, B_SIG, B_LEN, B_RAW, NB_FIELDS };

typedef struct {
  int kind;
  addon_ctx* c;
  bgv_batch b;
  bgv_bits_batch bb;    /* K_BITS (b.n_jobs / b.n_sets mirror its counts) */
  uint32_t* src_copy;   /* K_BITS: the sources, copied at call time like the offsets */
  napi_ref brefs[NB_FIELDS];
  uint8_t miller[576];  /* K_PARTIAL */
  int32_t ok;           /* K_PARTIAL: no job rejected; K_COMBINE: the product is 1 in GT */
  uint8_t* parts;       /* K_COMBINE: a copy of the partials */
  uint32_t n_parts;
  uint32_t* job_off; /* copies made at call time (the library reads these) */
  uint32_t* pk_off;
  int32_t* job_result;
  bgv_stats stats;
  bgv_hash_path hash_path; /* K_VERIFY, K_BITS, K_PARTIAL: read under the context's lock */
  bgv_pair_path pair_path; /* likewise */
  double t_start_ms, t_end_ms;
  int status;
  char err[512];
  napi_ref refs[N_FIELDS];
  napi_ref ctx_ref;
  napi_async_work work;
  napi_deferred deferred;
} verify_job;

static void free_job_arrays(verify_job* j) {
  free(j->job_off);
  free(j->pk_off);
  free(j->job_result);
  free(j->parts);
  free(j->src_copy);
  j->src_copy = NULL;
  j->job_off = j->pk_off = NULL;
  j->job_result = NULL;
  j->parts = NULL;
}

/* reads the batch object into j->b; copies the offsets; pins the other arrays when pin != 0 */
static int read_batch(napi_env env, napi_value obj, verify_job* j, int pin) {
  void* p[N_FIELDS] = {0};
  size_t n[N_FIELDS] = {0};
  napi_value v[N_FIELDS];
  for (int k = 0; k < N_FIELDS; k++) {
    bool has = false;
    napi_has_named_property(env, obj, FIELD[k], &has);
    if (!has) {
      if (k == F_RAW) continue;
      napi_throw_type_error(env, NULL, "batch field missing");
      return -1;
    }
    napi_get_named_property(env, obj, FIELD[k], &v[k]);
    if (typed(env, v[k], FIELD_T[k], &p[k], &n[k])) {
      napi_throw_type_error(env, NULL, "batch field has the wrong typed-array type");
      return -1;
    }
  }
  if (n[F_JOB] < 1 || n[F_PKO] < 1) {
    napi_throw_range_error(env, NULL, "jobOffsets / pkOffsets need at least one entry");
    return -1;
  }
  memset(&j->b, 0, sizeof j->b);
  j->b.n_jobs = (uint32_t)(n[F_JOB] - 1);
  j->b.n_sets = (uint32_t)(n[F_PKO] - 1);
  j->job_off = (uint32_t*)malloc(4 * n[F_JOB]);
  j->pk_off = (uint32_t*)malloc(4 * n[F_PKO]);
  if (!j->job_off || !j->pk_off) {
    napi_throw_error(env, NULL, "out of memory");
    return -1;
  }
  memcpy(j->job_off, p[F_JOB], 4 * n[F_JOB]);
  memcpy(j->pk_off, p[F_PKO], 4 * n[F_PKO]);
  const uint32_t n_sets = j->b.n_sets;
  if (n[F_MSG] < 32ull * n_sets || n[F_SIG] < 192ull * n_sets || n[F_LEN] < n_sets) {
    napi_throw_range_error(env, NULL, "msgs / sigs / sigLen shorter than the set count");
    return -1;
  }
  if (n[F_PKI] < (size_t)j->pk_off[n_sets]) {
    napi_throw_range_error(env, NULL, "pkIndices shorter than pkOffsets[n_sets]");
    return -1;
  }
  if (pin)
    for (int k = 0; k < N_FIELDS; k++)
      if (p[k] && k != F_JOB && k != F_PKO) napi_create_reference(env, v[k], 1, &j->refs[k]);
  j->b.job_offsets = j->job_off;
  j->b.pk_offsets = j->pk_off;
  j->b.pk_indices = (const uint32_t*)p[F_PKI];
  j->b.msgs = (const uint8_t*)p[F_MSG];
  j->b.sigs = (const uint8_t*)p[F_SIG];
  j->b.sig_len = (const uint32_t*)p[F_LEN];
  j->b.raw_pks = (const uint8_t*)p[F_RAW];
  j->b.n_raw = (uint32_t)(n[F_RAW] / 96);
  j->b.scalars = NULL; /* drawn inside the library (device ChaCha20 keyed by getrandom) */
  j->b.on_device = 0;
  return 0;
}

static double now_ms(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec * 1e3 + (double)t.tv_nsec * 1e-6;
}

static void run_verify(verify_job* j) {
  pthread_mutex_lock(&j->c->mu);
  j->t_start_ms = now_ms();
  if (j->c->closed) {
    j->status = BGV_E_INVALID_ARG;
    snprintf(j->err, sizeof j->err, "QUEUE_ERROR_QUEUE_ABORTED");
  } else {
    switch (j->kind) {
      case K_PARTIAL:
        j->status = bgv_partial(j->c->ctx, &j->b, j->miller, NULL, j->job_result, &j->ok);
        j->c->partial_jobs = j->b.n_jobs;
        if (j->status == BGV_OK) {
          j->status = bgv_last_stats(j->c->ctx, &j->stats);
          j->stats.pubkeys_aggregated = j->b.n_sets ? j->pk_off[j->b.n_sets] : 0;
        }
        break;
      case K_FINISH:
        j->b.n_jobs = j->c->partial_jobs;
        j->job_result = (int32_t*)calloc(j->b.n_jobs ? j->b.n_jobs : 1, 4);
        j->status = j->job_result ? bgv_partial_finish(j->c->ctx, j->job_result, &j->stats) : BGV_E_INVALID_ARG;
        break;
      case K_COMBINE: j->status = bgv_combine_final(j->c->ctx, j->parts, j->n_parts, &j->ok); break;
      case K_BITS: j->status = bgv_verify_bits(j->c->ctx, &j->bb, j->job_result, NULL, &j->stats); break;
      default: j->status = bgv_verify(j->c->ctx, &j->b, j->job_result, NULL, &j->stats); break;
    }
    /* under the same lock: this call's evaluations, not a later call's */
    if (j->status == BGV_OK && (j->kind == K_VERIFY || j->kind == K_BITS || j->kind == K_PARTIAL))
      j->status = bgv_hash_stats(j->c->ctx, &j->hash_path);
    if (j->status == BGV_OK && (j->kind == K_VERIFY || j->kind == K_BITS || j->kind == K_PARTIAL))
      j->status = bgv_pair_stats(j->c->ctx, &j->pair_path);
    if (j->status != BGV_OK) snprintf(j->err, sizeof j->err, "bgv error %d: %s", j->status, bgv_last_error());
  }
  j->t_end_ms = now_ms();
  pthread_mutex_unlock(&j->c->mu);
}

/* {results, batchRetries, batchSigsSuccess, pubkeysAggregated, deviceMs, workerStartMs, workerEndMs} */
static napi_value result_object(napi_env env, const verify_job* j) {
  napi_value o, v;
  if (napi_create_object(env, &o) != napi_ok) return NULL;
  v = new_int32_array(env, j->job_result, j->b.n_jobs);
  if (!v) return NULL;
  napi_set_named_property(env, o, "results", v);
  napi_create_uint32(env, j->stats.batch_retries, &v);
  napi_set_named_property(env, o, "batchRetries", v);
  napi_create_uint32(env, j->stats.batch_sigs_success, &v);
  napi_set_named_property(env, o, "batchSigsSuccess", v);
  napi_create_double(env, (double)j->stats.pubkeys_aggregated, &v);
  napi_set_named_property(env, o, "pubkeysAggregated", v);
  napi_create_double(env, (double)j->stats.total_ms, &v);
  napi_set_named_property(env, o, "deviceMs", v);
  napi_create_double(env, j->t_start_ms, &v);
  napi_set_named_property(env, o, "workerStartMs", v);
  napi_create_double(env, j->t_end_ms, &v);
  napi_set_named_property(env, o, "workerEndMs", v);
  if (j->kind == K_VERIFY || j->kind == K_BITS || j->kind == K_PARTIAL) {
    napi_create_uint32(env, j->hash_path.hashes, &v);
    napi_set_named_property(env, o, "hashes", v);
    napi_create_uint32(env, j->pair_path.pairs, &v);
    napi_set_named_property(env, o, "millerPairs", v);
  }
  if (j->kind == K_PARTIAL) {
    void* dst = NULL;
    napi_value ab;
    if (napi_create_arraybuffer(env, 576, &dst, &ab) != napi_ok) return NULL;
    memcpy(dst, j->miller, 576);
    napi_create_typedarray(env, napi_uint8_array, 576, ab, 0, &v);
    napi_set_named_property(env, o, "miller", v);
    napi_get_boolean(env, j->ok != 0, &v);
    napi_set_named_property(env, o, "ok", v);
  }
  return o;
}

static void exec_verify(napi_env env, void* data) { /* libuv worker thread */
  (void)env;
  run_verify((verify_job*)data);
}

static void done_verify(napi_env env, napi_status st, void* data) { /* main thread */
  verify_job* j = (verify_job*)data;
  if (st != napi_ok && j->status == BGV_OK) {
    j->status = BGV_E_INVALID_ARG;
    snprintf(j->err, sizeof j->err, "async work cancelled");
  }
  if (j->status != BGV_OK) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->err, NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->kind == K_COMBINE) {
    napi_value b;
    napi_get_boolean(env, j->ok != 0, &b);
    napi_resolve_deferred(env, j->deferred, b);
  } else {
    napi_resolve_deferred(env, j->deferred, result_object(env, j));
  }
  for (int k = 0; k < N_FIELDS; k++)
    if (j->refs[k]) napi_delete_reference(env, j->refs[k]); /* unpin the inputs */
  for (int k = 0; k < NB_FIELDS; k++)
    if (j->brefs[k]) napi_delete_reference(env, j->brefs[k]);
  if (j->ctx_ref) napi_delete_reference(env, j->ctx_ref);
  napi_delete_async_work(env, j->work);
  free_job_arrays(j);
  free(j);
}

/* queue j on the libuv pool; the promise settles in done_verify */
static napi_value queue_job(napi_env env, napi_value ctx_val, verify_job* j, const char* label) {
  napi_create_reference(env, ctx_val, 1, &j->ctx_ref); /* the context outlives its queued work */
  napi_value promise, name;
  NAPI_CALL(env, napi_create_promise(env, &j->deferred, &promise));
  NAPI_CALL(env, napi_create_string_utf8(env, label, NAPI_AUTO_LENGTH, &name));
  NAPI_CALL(env, napi_create_async_work(env, NULL, name, exec_verify, done_verify, j, &j->work));
  NAPI_CALL(env, napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value queue_batch(napi_env env, napi_callback_info info, int kind, const char* label) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  verify_job* j = (verify_job*)calloc(1, sizeof *j);
  j->c = c;
  j->kind = kind;
  if (read_batch(env, a[1], j, 1)) {
    for (int k = 0; k < N_FIELDS; k++)
      if (j->refs[k]) napi_delete_reference(env, j->refs[k]);
    free_job_arrays(j);
    free(j);
    return NULL;
  }
  j->job_result = (int32_t*)calloc(j->b.n_jobs ? j->b.n_jobs : 1, 4);
  return queue_job(env, a[0], j, label);
}

static napi_value Verify(napi_env env, napi_callback_info info) { return queue_batch(env, info, K_VERIFY, "bgv_verify"); }

static napi_value Partial(napi_env env, napi_callback_info info) { return queue_batch(env, info, K_PARTIAL, "bgv_partial"); }

/* partialFinish(ctx): the shard left by the last partial() on the context */
static napi_value PartialFinish(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  verify_job* j = (verify_job*)calloc(1, sizeof *j);
  j->c = c;
  j->kind = K_FINISH; /* results sized on the pool thread from the pending partial */
  return queue_job(env, a[0], j, "bgv_partial_finish");
}

static napi_value CombineFinal(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  void* data;
  size_t len;
  if (argc < 2 || typed(env, a[1], napi_uint8_array, &data, &len) || len % 576) {
    napi_throw_type_error(env, NULL, "combineFinal(ctx, Uint8Array of 576-byte partials)");
    return NULL;
  }
  verify_job* j = (verify_job*)calloc(1, sizeof *j);
  j->c = c;
  j->kind = K_COMBINE;
  j->n_parts = (uint32_t)(len / 576);
  j->parts = (uint8_t*)malloc(len ? len : 1); /* copied: the caller may reuse its buffer */
  if (len) memcpy(j->parts, data, len);
  return queue_job(env, a[0], j, "bgv_combine_final");
}

static napi_value VerifySync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  verify_job j;
  memset(&j, 0, sizeof j);
  j.c = c;
  if (read_batch(env, a[1], &j, 0)) {
    free_job_arrays(&j);
    return NULL;
  }
  j.job_result = (int32_t*)calloc(j.b.n_jobs ? j.b.n_jobs : 1, 4);
  run_verify(&j);
  napi_value r = NULL;
  if (j.status != BGV_OK) napi_throw_error(env, NULL, j.err);
  else r = result_object(env, &j);
  free_job_arrays(&j);
  return r;
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
enum { S_GRP, S_PKI, S_MSG, S_SIG, S_LEN, S_RAW, S_PKO, S_SRC, S_BITS, S_FIELDS }; /* S_SRC on: verifySameMessageBits only */
static const char* SM_FIELD[S_FIELDS] = {"groupOffsets", "pkIndices", "msgs", "sigs", "sigLen", "rawPks", "pkOffsets", "src", "bits"};
static const napi_typedarray_type SM_FIELD_T[S_FIELDS] = {napi_uint32_array, napi_uint32_array, napi_uint8_array,
                                                          napi_uint8_array,  napi_uint32_array, napi_uint8_array,
                                                          napi_uint32_array, napi_uint32_array, napi_uint8_array};

typedef struct {
  addon_ctx* c;
  bgv_sm_batch b;
  int agg;          /* 1: the sets' keys are aggregates: `ba` is the batch, `b` keeps the counts;
                       2: ... given as committee sets: `bb` is the batch (verifySameMessageBits) */
  bgv_sma_batch ba;
  bgv_smb_batch bb;
  uint32_t* src_copy;
  bgv_bits_path path; /* agg == 2: the path counters of the call */
  int with_sums;      /* verifySameMessageAggregate (agg == 0): `ag` and its three outputs */
  bgv_sm_agg ag;
  uint8_t* agg_sigs;
  uint32_t* agg_count;
  int32_t* agg_code;
  napi_ref sum_refs[2]; /* take, prevSigs */
  uint32_t* pk_off;
  uint32_t* group_off;
  uint8_t* valid;
  int32_t* codes;
  bgv_sm_stats stats;
  double t_start_ms, t_end_ms;
  int status;
  char err[512];
  napi_ref refs[S_FIELDS];
  napi_ref ctx_ref;
  napi_async_work work;
  napi_deferred deferred;
} sm_job;

static void sm_free(napi_env env, sm_job* j) {
  for (int k = 0; k < S_FIELDS; k++)
    if (j->refs[k]) napi_delete_reference(env, j->refs[k]);
  if (j->ctx_ref) napi_delete_reference(env, j->ctx_ref);
  free(j->group_off);
  free(j->pk_off);
  free(j->src_copy);
  free(j->valid);
  free(j->codes);
  for (int k = 0; k < 2; k++)
    if (j->sum_refs[k]) napi_delete_reference(env, j->sum_refs[k]);
  free(j->agg_sigs);
  free(j->agg_count);
  free(j->agg_code);
}

static int sm_read_batch(napi_env env, napi_value obj, sm_job* j, int pin) {
  void* p[S_FIELDS] = {0};
  size_t n[S_FIELDS] = {0};
  napi_value v[S_FIELDS];
  for (int k = 0; k < S_SRC; k++) {
    bool has = false;
    if (k == S_PKO && !j->agg) continue;
    napi_has_named_property(env, obj, SM_FIELD[k], &has);
    if (!has) {
      if (k == S_RAW) continue;
      napi_throw_type_error(env, NULL, "batch field missing");
      return -1;
    }
    napi_get_named_property(env, obj, SM_FIELD[k], &v[k]);
    if (typed(env, v[k], SM_FIELD_T[k], &p[k], &n[k])) {
      napi_throw_type_error(env, NULL, "batch field has the wrong typed-array type");
      return -1;
    }
  }
  if (n[S_GRP] < 1) {
    napi_throw_range_error(env, NULL, "groupOffsets needs at least one entry");
    return -1;
  }
  memset(&j->b, 0, sizeof j->b);
  j->b.n_groups = (uint32_t)(n[S_GRP] - 1);
  j->group_off = (uint32_t*)malloc(4 * n[S_GRP]);
  if (!j->group_off) {
    napi_throw_error(env, NULL, "out of memory");
    return -1;
  }
  memcpy(j->group_off, p[S_GRP], 4 * n[S_GRP]);
  const uint32_t n_sets = j->group_off[j->b.n_groups];
  j->b.n_sets = n_sets;
  size_t n_keys = n_sets;
  if (j->agg) {
    if (n[S_PKO] < (size_t)n_sets + 1) {
      napi_throw_range_error(env, NULL, "pkOffsets shorter than the set count + 1");
      return -1;
    }
    j->pk_off = (uint32_t*)malloc(4 * ((size_t)n_sets + 1));
    if (!j->pk_off) {
      napi_throw_error(env, NULL, "out of memory");
      return -1;
    }
    memcpy(j->pk_off, p[S_PKO], 4 * ((size_t)n_sets + 1));
    n_keys = j->pk_off[n_sets];
  }
  if (n[S_MSG] < 32ull * j->b.n_groups || n[S_SIG] < 192ull * n_sets || n[S_LEN] < n_sets || n[S_PKI] < n_keys) {
    napi_throw_range_error(env, NULL, "msgs / sigs / sigLen / pkIndices shorter than the group, set or key count");
    return -1;
  }
  j->valid = (uint8_t*)calloc(n_sets ? n_sets : 1, 1);
  j->codes = (int32_t*)calloc(n_sets ? n_sets : 1, 4);
  if (!j->valid || !j->codes) {
    napi_throw_error(env, NULL, "out of memory");
    return -1;
  }
  if (pin)
    for (int k = 0; k < S_SRC; k++)
      if (p[k] && k != S_GRP && k != S_PKO) napi_create_reference(env, v[k], 1, &j->refs[k]);
  j->b.group_offsets = j->group_off;
  j->b.pk_indices = (const uint32_t*)p[S_PKI];
  j->b.msgs = (const uint8_t*)p[S_MSG];
  j->b.sigs = (const uint8_t*)p[S_SIG];
  j->b.sig_len = (const uint32_t*)p[S_LEN];
  j->b.raw_pks = (const uint8_t*)p[S_RAW];
  j->b.n_raw = (uint32_t)(n[S_RAW] / 96);
  j->b.scalars = NULL; /* drawn inside the library */
  j->b.on_device = 0;
  if (j->with_sums) {
    static const char* name[2] = {"take", "prevSigs"};
    const size_t need[2] = {n_sets, 96ull * j->b.n_groups};
    const void* q[2] = {NULL, NULL};
    for (int k = 0; k < 2; k++) {
      bool has = false;
      napi_value val;
      napi_valuetype vt;
      size_t len = 0;
      void* ptr = NULL;
      napi_has_named_property(env, obj, name[k], &has);
      if (!has) continue;
      napi_get_named_property(env, obj, name[k], &val);
      napi_typeof(env, val, &vt);
      if (vt == napi_undefined || vt == napi_null) continue;
      if (typed(env, val, napi_uint8_array, &ptr, &len)) {
        napi_throw_type_error(env, NULL, "take / prevSigs must be a Uint8Array");
        return -1;
      }
      if (len < need[k]) {
        napi_throw_range_error(env, NULL, "take / prevSigs shorter than the set / group count");
        return -1;
      }
      q[k] = ptr;
      if (pin) napi_create_reference(env, val, 1, &j->sum_refs[k]);
    }
    const size_t G = j->b.n_groups ? j->b.n_groups : 1;
    j->agg_sigs = (uint8_t*)calloc(G, 96);
    j->agg_count = (uint32_t*)calloc(G, 4);
    j->agg_code = (int32_t*)calloc(G, 4);
    if (!j->agg_sigs || !j->agg_count || !j->agg_code) {
      napi_throw_error(env, NULL, "out of memory");
      return -1;
    }
    j->ag.take = (const uint8_t*)q[0];
    j->ag.prev_sig96 = (const uint8_t*)q[1];
    j->ag.agg_sig96 = j->agg_sigs;
    j->ag.agg_count = j->agg_count;
    j->ag.agg_code = j->agg_code;
  }
  if (j->agg) {
    memset(&j->ba, 0, sizeof j->ba);
    j->ba.n_sets = n_sets;
    j->ba.n_groups = j->b.n_groups;
    j->ba.group_offsets = j->group_off;
    j->ba.pk_offsets = j->pk_off;
    j->ba.pk_indices = j->b.pk_indices;
    j->ba.raw_pks = j->b.raw_pks;
    j->ba.n_raw = j->b.n_raw;
    j->ba.msgs = j->b.msgs;
    j->ba.sigs = j->b.sigs;
    j->ba.sig_len = j->b.sig_len;
  }
  return 0;
}

/* verifySameMessageBits(ctx, batch) -> Promise<result>, verifySameMessageBitsSync(ctx, batch) -> result
 * (bgv_verify_same_message_bits).  batch = {groupOffsets, src: Uint32Array (4 per set, as verifyBits), bits:
 * Uint8Array, pkIndices: Uint32Array (keys of the explicit sets), msgs (32 B per GROUP), sigs, sigLen, rawPks?}.
 * result as verifySameMessageAgg plus pubkeysAggregated, the participating keys from the call's path counters
 * (the caller holds no index lists to count them from).  Ownership as for verifyBits: groupOffsets and src are
 * copied at call time, the other typed arrays are pinned until completion. */
static int smb_read_batch(napi_env env, napi_value obj, sm_job* j, int pin) {
  void* p[S_FIELDS] = {0};
  size_t n[S_FIELDS] = {0};
  napi_value v[S_FIELDS];
  for (int k = 0; k < S_FIELDS; k++) {
    bool has = false;
    if (k == S_PKO) continue;
    napi_has_named_property(env, obj, SM_FIELD[k], &has);
    if (!has) {
      if (k == S_RAW) continue;
      napi_throw_type_error(env, NULL, "batch field missing");
      return -1;
    }
    napi_get_named_property(env, obj, SM_FIELD[k], &v[k]);
    if (typed(env, v[k], SM_FIELD_T[k], &p[k], &n[k])) {
      napi_throw_type_error(env, NULL, "batch field has the wrong typed-array type");
      return -1;
    }
  }
  if (n[S_GRP] < 1 || n[S_SRC] % 4) {
    napi_throw_range_error(env, NULL, "groupOffsets needs at least one entry, src four entries per set");
    return -1;
  }
  const size_t n_sets = n[S_SRC] / 4;
  if (n_sets > 0xffffffffull || n[S_BITS] > 0xffffffffull || n[S_PKI] > 0xffffffffull) {
    napi_throw_range_error(env, NULL, "bits batch too large");
    return -1;
  }
  memset(&j->b, 0, sizeof j->b);
  j->b.n_groups = (uint32_t)(n[S_GRP] - 1);
  j->b.n_sets = (uint32_t)n_sets;
  j->group_off = (uint32_t*)malloc(4 * n[S_GRP]);
  j->src_copy = (uint32_t*)malloc(n[S_SRC] ? 4 * n[S_SRC] : 4);
  if (!j->group_off || !j->src_copy) {
    napi_throw_error(env, NULL, "out of memory");
    return -1;
  }
  memcpy(j->group_off, p[S_GRP], 4 * n[S_GRP]);
  if (n[S_SRC]) memcpy(j->src_copy, p[S_SRC], 4 * n[S_SRC]);
  if (j->group_off[j->b.n_groups] != n_sets) {
    napi_throw_range_error(env, NULL, "groupOffsets must end at the set count of src");
    return -1;
  }
  if (n[S_MSG] < 32ull * j->b.n_groups || n[S_SIG] < 192ull * n_sets || n[S_LEN] < n_sets) {
    napi_throw_range_error(env, NULL, "msgs / sigs / sigLen shorter than the group or set count");
    return -1;
  }
  j->valid = (uint8_t*)calloc(n_sets ? n_sets : 1, 1);
  j->codes = (int32_t*)calloc(n_sets ? n_sets : 1, 4);
  if (!j->valid || !j->codes) {
    napi_throw_error(env, NULL, "out of memory");
    return -1;
  }
  if (pin)
    for (int k = 0; k < S_FIELDS; k++)
      if (p[k] && k != S_GRP && k != S_SRC) napi_create_reference(env, v[k], 1, &j->refs[k]);
  memset(&j->bb, 0, sizeof j->bb);
  j->bb.n_sets = (uint32_t)n_sets;
  j->bb.n_groups = j->b.n_groups;
  j->bb.group_offsets = j->group_off;
  j->bb.src = (const bgv_set_src*)j->src_copy;
  j->bb.bits = (const uint8_t*)p[S_BITS];
  j->bb.bits_len = (uint32_t)n[S_BITS];
  j->bb.pk_indices = (const uint32_t*)p[S_PKI];
  j->bb.n_indices = (uint32_t)n[S_PKI];
  j->bb.raw_pks = (const uint8_t*)p[S_RAW];
  j->bb.n_raw = (uint32_t)(n[S_RAW] / 96);
  j->bb.msgs = (const uint8_t*)p[S_MSG];
  j->bb.sigs = (const uint8_t*)p[S_SIG];
  j->bb.sig_len = (const uint32_t*)p[S_LEN];
  j->bb.scalars = NULL; /* drawn inside the library */
  j->bb.on_device = 0;
  return 0;
}

static void sm_run(sm_job* j) {
  pthread_mutex_lock(&j->c->mu);
  j->t_start_ms = now_ms();
  if (j->c->closed) {
    j->status = BGV_E_INVALID_ARG;
    snprintf(j->err, sizeof j->err, "QUEUE_ERROR_QUEUE_ABORTED");
  } else {
    if (j->agg == 2) {
      j->status = bgv_verify_same_message_bits(j->c->ctx, &j->bb, j->valid, j->codes, &j->stats);
      if (j->status == BGV_OK) j->status = bgv_bits_path_stats(j->c->ctx, &j->path); /* under the same lock: this call's */
    } else {
      j->status = j->agg         ? bgv_verify_same_message_agg(j->c->ctx, &j->ba, j->valid, j->codes, &j->stats)
                  : j->with_sums ? bgv_verify_same_message_aggregate(j->c->ctx, &j->b, &j->ag, j->valid, j->codes, &j->stats)
                                 : bgv_verify_same_message(j->c->ctx, &j->b, j->valid, j->codes, &j->stats);
    }
    if (j->status != BGV_OK) snprintf(j->err, sizeof j->err, "bgv error %d: %s", j->status, bgv_last_error());
  }
  j->t_end_ms = now_ms();
  pthread_mutex_unlock(&j->c->mu);
}

static napi_value sm_result(napi_env env, const sm_job* j) {
  napi_value o, v, ab;
  void* dst = NULL;
  if (napi_create_object(env, &o) != napi_ok) return NULL;
  if (napi_create_arraybuffer(env, j->b.n_sets, &dst, &ab) != napi_ok) return NULL;
  if (j->b.n_sets) memcpy(dst, j->valid, j->b.n_sets);
  napi_create_typedarray(env, napi_uint8_array, j->b.n_sets, ab, 0, &v);
  napi_set_named_property(env, o, "valid", v);
  v = new_int32_array(env, j->codes, j->b.n_sets);
  if (!v) return NULL;
  napi_set_named_property(env, o, "codes", v);
  const struct { const char* name; uint32_t val; } u[] = {
      {"segments", j->stats.n_segments}, {"hashes", j->stats.hashes}, {"pairs", j->stats.pairs},
      {"groupsRetried", j->stats.groups_retried}, {"setsRetried", j->stats.sets_retried}};
  for (size_t k = 0; k < sizeof u / sizeof u[0]; k++) {
    napi_create_uint32(env, u[k].val, &v);
    napi_set_named_property(env, o, u[k].name, v);
  }
  if (j->agg == 2) {
    napi_create_uint32(env, j->path.keys_expanded, &v);
    napi_set_named_property(env, o, "pubkeysAggregated", v);
  }
  if (j->with_sums) {
    const size_t G = j->b.n_sets ? j->b.n_groups : 0; /* an empty batch writes nothing */
    if (napi_create_arraybuffer(env, 96 * G, &dst, &ab) != napi_ok) return NULL;
    if (G) memcpy(dst, j->agg_sigs, 96 * G);
    napi_create_typedarray(env, napi_uint8_array, 96 * G, ab, 0, &v);
    napi_set_named_property(env, o, "aggSigs", v);
    if (napi_create_arraybuffer(env, 4 * G, &dst, &ab) != napi_ok) return NULL;
    if (G) memcpy(dst, j->agg_count, 4 * G);
    napi_create_typedarray(env, napi_uint32_array, G, ab, 0, &v);
    napi_set_named_property(env, o, "aggCount", v);
    v = new_int32_array(env, j->agg_code, G);
    if (!v) return NULL;
    napi_set_named_property(env, o, "aggCode", v);
  }
  napi_create_double(env, (double)j->stats.total_ms, &v);
  napi_set_named_property(env, o, "deviceMs", v);
  napi_create_double(env, j->t_start_ms, &v);
  napi_set_named_property(env, o, "workerStartMs", v);
  napi_create_double(env, j->t_end_ms, &v);
  napi_set_named_property(env, o, "workerEndMs", v);
  return o;
}

static void sm_exec(napi_env env, void* data) { /* libuv worker thread */
  (void)env;
  sm_run((sm_job*)data);
}

static void sm_done(napi_env env, napi_status st, void* data) { /* main thread */
  sm_job* j = (sm_job*)data;
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
    napi_resolve_deferred(env, j->deferred, sm_result(env, j));
  }
  napi_delete_async_work(env, j->work);
  sm_free(env, j);
  free(j);
}

static napi_value sm_async(napi_env env, napi_callback_info info, int agg) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  sm_job* j = (sm_job*)calloc(1, sizeof *j);
  j->c = c;
  j->with_sums = agg == 3;
  if (agg == 3) agg = 0;
  j->agg = agg;
  if (agg == 2 ? smb_read_batch(env, a[1], j, 1) : sm_read_batch(env, a[1], j, 1)) {
    sm_free(env, j);
    free(j);
    return NULL;
  }
  napi_create_reference(env, a[0], 1, &j->ctx_ref); /* the context outlives its queued work */
  napi_value promise, name;
  NAPI_CALL(env, napi_create_promise(env, &j->deferred, &promise));
  NAPI_CALL(env, napi_create_string_utf8(env, agg == 2 ? "bgv_verify_same_message_bits" : agg ? "bgv_verify_same_message_agg" : j->with_sums ? "bgv_verify_same_message_aggregate" : "bgv_verify_same_message",
                                         NAPI_AUTO_LENGTH, &name));
  NAPI_CALL(env, napi_create_async_work(env, NULL, name, sm_exec, sm_done, j, &j->work));
  NAPI_CALL(env, napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value sm_sync(napi_env env, napi_callback_info info, int agg) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  sm_job j;
  memset(&j, 0, sizeof j);
  j.c = c;
  j.with_sums = agg == 3;
  if (agg == 3) agg = 0;
  j.agg = agg;
  napi_value r = NULL;
  if (!(agg == 2 ? smb_read_batch(env, a[1], &j, 0) : sm_read_batch(env, a[1], &j, 0))) {
    sm_run(&j);
    if (j.status != BGV_OK) napi_throw_error(env, NULL, j.err);
    else r = sm_result(env, &j);
  }
  sm_free(env, &j);
  return r;
}

static napi_value VerifySameMessage(napi_env env, napi_callback_info info) { return sm_async(env, info, 0); }
static napi_value VerifySameMessageSync(napi_env env, napi_callback_info info) { return sm_sync(env, info, 0); }
static napi_value VerifySameMessageAgg(napi_env env, napi_callback_info info) { return sm_async(env, info, 1); }
static napi_value VerifySameMessageAggSync(napi_env env, napi_callback_info info) { return sm_sync(env, info, 1); }
static napi_value VerifySameMessageAggregate(napi_env env, napi_callback_info info) { return sm_async(env, info, 3); }
static napi_value VerifySameMessageAggregateSync(napi_env env, napi_callback_info info) { return sm_sync(env, info, 3); }
static napi_value VerifySameMessageBits(napi_env env, napi_callback_info info) { return sm_async(env, info, 2); }
static napi_value VerifySameMessageBitsSync(napi_env env, napi_callback_info info) { return sm_sync(env, info, 2); }

/* ------------------------------------------------------- committee bitfields
 * verifyBits(ctx, batch) -> Promise<result>, verifyBitsSync(ctx, batch) -> result (bgv_verify_bits).
 * batch = {jobOffsets: Uint32Array, src: Uint32Array (4 per set: list, off, len, bitsOff; list 0xffffffff = an
 * explicit run pkIndices[off .. off + len)), bits: Uint8Array (all bitfields, byte-packed, SSZ bit order),
 * pkIndices: Uint32Array (keys of the explicit sets), msgs, sigs, sigLen, rawPks? as for verify}.
 * result as for verify.  jobOffsets and src are copied at call time; the library stages every array into pinned
 * memory and checks the copy against the lengths taken here, so a caller that mutates its arrays while the work
 * is queued cannot make the device read past them. */
static const char* BFIELD[NB_FIELDS] = {"jobOffsets", "src", "bits", "pkIndices", "msgs", "sigs", "sigLen", "rawPks"};
static const napi_typedarray_type BFIELD_T[NB_FIELDS] = {napi_uint32_array, napi_uint32_array, napi_uint8_array,  napi_uint32_array,
                                                         napi_uint8_array,  napi_uint8_array,  napi_uint32_array, napi_uint8_array};

static int read_bits_batch(napi_env env, napi_value obj, verify_job* j, int pin) {
  void* p[NB_FIELDS] = {0};
  size_t n[NB_FIELDS] = {0};
  napi_value v[NB_FIELDS];
  for (int k = 0; k < NB_FIELDS; k++) {
    bool has = false;
    napi_has_named_property(env, obj, BFIELD[k], &has);
    if (!has) {
      if (k == B_RAW) continue;
      napi_throw_type_error(env, NULL, "bits batch field missing");
      return -1;
    }
    napi_get_named_property(env, obj, BFIELD[k], &v[k]);
    if (typed(env, v[k], BFIELD_T[k], &p[k], &n[k])) {
      napi_throw_type_error(env, NULL, "bits batch field has the wrong typed-array type");
      return -1;
    }
  }
  if (n[B_JOB] < 1 || n[B_SRC] % 4) {
    napi_throw_range_error(env, NULL, "jobOffsets needs at least one entry, src four entries per set");
    return -1;
  }
  const size_t n_sets = n[B_SRC] / 4;
  if (n[B_MSG] < 32ull * n_sets || n[B_SIG] < 192ull * n_sets || n[B_LEN] < n_sets) {
    napi_throw_range_error(env, NULL, "msgs / sigs / sigLen shorter than the set count");
    return -1;
  }
  if (n_sets > 0xffffffffull || n[B_BITS] > 0xffffffffull || n[B_PKI] > 0xffffffffull) {
    napi_throw_range_error(env, NULL, "bits batch too large");
    return -1;
  }
  j->job_off = (uint32_t*)malloc(4 * n[B_JOB]);
  j->src_copy = (uint32_t*)malloc(n[B_SRC] ? 4 * n[B_SRC] : 4);
  if (!j->job_off || !j->src_copy) {
    napi_throw_error(env, NULL, "out of memory");
    return -1;
  }
  memcpy(j->job_off, p[B_JOB], 4 * n[B_JOB]);
  if (n[B_SRC]) memcpy(j->src_copy, p[B_SRC], 4 * n[B_SRC]);
  if (pin)
    for (int k = 0; k < NB_FIELDS; k++)
      if (p[k] && k != B_JOB && k != B_SRC) napi_create_reference(env, v[k], 1, &j->brefs[k]);
  memset(&j->bb, 0, sizeof j->bb);
  j->bb.n_sets = (uint32_t)n_sets;
  j->bb.n_jobs = (uint32_t)(n[B_JOB] - 1);
  j->bb.job_offsets = j->job_off;
  j->bb.src = (const bgv_set_src*)j->src_copy;
  j->bb.bits = (const uint8_t*)p[B_BITS];
  j->bb.bits_len = (uint32_t)n[B_BITS];
  j->bb.pk_indices = (const uint32_t*)p[B_PKI];
  j->bb.n_indices = (uint32_t)n[B_PKI];
  j->bb.raw_pks = (const uint8_t*)p[B_RAW];
  j->bb.n_raw = (uint32_t)(n[B_RAW] / 96);
  j->bb.msgs = (const uint8_t*)p[B_MSG];
  j->bb.sigs = (const uint8_t*)p[B_SIG];
  j->bb.sig_len = (const uint32_t*)p[B_LEN];
  j->bb.scalars = NULL; /* drawn inside the library */
  j->bb.on_device = 0;
  j->b.n_jobs = j->bb.n_jobs; /* result_object sizes `results` from it */
  j->b.n_sets = j->bb.n_sets;
  return 0;
}

static napi_value VerifyBits(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  verify_job* j = (verify_job*)calloc(1, sizeof *j);
  j->c = c;
  j->kind = K_BITS;
  if (read_bits_batch(env, a[1], j, 1)) {
    for (int k = 0; k < NB_FIELDS; k++)
      if (j->brefs[k]) napi_delete_reference(env, j->brefs[k]);
    free_job_arrays(j);
    free(j);
    return NULL;
  }
  j->job_result = (int32_t*)calloc(j->b.n_jobs ? j->b.n_jobs : 1, 4);
  return queue_job(env, a[0], j, "bgv_verify_bits");
}

static napi_value VerifyBitsSync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  verify_job j;
  memset(&j, 0, sizeof j);
  j.c = c;
  j.kind = K_BITS;
  if (read_bits_batch(env, a[1], &j, 0)) {
    free_job_arrays(&j);
    return NULL;
  }
  j.job_result = (int32_t*)calloc(j.b.n_jobs ? j.b.n_jobs : 1, 4);
  run_verify(&j);
  napi_value r = NULL;
  if (j.status != BGV_OK) napi_throw_error(env, NULL, j.err);
  else r = result_object(env, &j);
  free_job_arrays(&j);
  return r;
}

static napi_value SetIndexList(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value a[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  uint32_t id = 0;
  void* data = NULL;
  size_t len = 0;
  if (argc < 3 || napi_get_value_uint32(env, a[1], &id) != napi_ok || typed(env, a[2], napi_uint32_array, &data, &len) ||
      len > 0xffffffffull) {
    napi_throw_type_error(env, NULL, "setIndexList(ctx, id, Uint32Array)");
    return NULL;
  }
  pthread_mutex_lock(&c->mu); /* waits for the context's batch in flight */
  const int st = bgv_index_list_set(c->ctx, id, (const uint32_t*)data, (uint32_t)len);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

static napi_value IndexListLen(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  uint32_t id = 0, n = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, a[1], &id));
  pthread_mutex_lock(&c->mu);
  const int st = bgv_index_list_len(c->ctx, id, &n);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r;
  NAPI_CALL(env, napi_create_uint32(env, n, &r));
  return r;
}

static napi_value SetIndexListSums(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value a[3];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  uint32_t id = 0;
  bool enable = false;
  if (argc < 3 || napi_get_value_uint32(env, a[1], &id) != napi_ok || napi_get_value_bool(env, a[2], &enable) != napi_ok) {
    napi_throw_type_error(env, NULL, "setIndexListSums(ctx, id, boolean)");
    return NULL;
  }
  pthread_mutex_lock(&c->mu); /* waits for the context's batch in flight */
  const int st = bgv_index_list_sums(c->ctx, id, enable ? 1u : 0u);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

static napi_value IndexListHasSums(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  uint32_t id = 0, has = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, a[1], &id));
  pthread_mutex_lock(&c->mu);
  const int st = bgv_index_list_has_sums(c->ctx, id, &has);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r;
  NAPI_CALL(env, napi_get_boolean(env, has != 0, &r));
  return r;
}

/* hashStats(ctx): bgv_hash_stats of the context's last ordinary batch (the sync paths read it after the call) */
static napi_value HashStats(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  bgv_hash_path p;
  pthread_mutex_lock(&c->mu);
  const int st = bgv_hash_stats(c->ctx, &p);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r, v;
  NAPI_CALL(env, napi_create_object(env, &r));
  NAPI_CALL(env, napi_create_uint32(env, p.sets, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "sets", v));
  NAPI_CALL(env, napi_create_uint32(env, p.hashes, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "hashes", v));
  NAPI_CALL(env, napi_create_uint32(env, p.dedup, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "dedup", v));
  return r;
}

/* pairMerge(ctx, on): bgv_pair_merge (a boolean, or 0 / 1; any other number is refused by the library) */
static napi_value PairMerge(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
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
  pthread_mutex_lock(&c->mu);
  const int st = bgv_pair_merge(c->ctx, mode);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

/* pairStats(ctx): bgv_pair_stats of the context's last ordinary batch */
static napi_value PairStats(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  bgv_pair_path p;
  pthread_mutex_lock(&c->mu);
  const int st = bgv_pair_stats(c->ctx, &p);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r, v;
  NAPI_CALL(env, napi_create_object(env, &r));
  NAPI_CALL(env, napi_create_uint32(env, p.sets, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "sets", v));
  NAPI_CALL(env, napi_create_uint32(env, p.pairs, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "pairs", v));
  NAPI_CALL(env, napi_create_uint32(env, p.merged, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "merged", v));
  NAPI_CALL(env, napi_create_uint32(env, p.fallback, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "fallback", v));
  return r;
}

/* smRetry(ctx, mode): bgv_sm_retry (a boolean, or 0 / 1; any other number is refused by the library) */
static napi_value SmRetry(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value a[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
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
  pthread_mutex_lock(&c->mu);
  const int st = bgv_sm_retry(c->ctx, mode);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  return NULL;
}

/* smRetryStats(ctx): bgv_sm_retry_stats of the context's last same-message call */
static napi_value SmRetryStats(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  bgv_sm_retry_path p;
  pthread_mutex_lock(&c->mu);
  const int st = bgv_sm_retry_stats(c->ctx, &p);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  const struct { const char* name; uint32_t val; } u[] = {
      {"mode", p.mode}, {"segments", p.segments}, {"subs", p.subs}, {"subsFailed", p.subs_failed},
      {"leaves", p.leaves}, {"pairs", p.pairs}, {"hashes", p.hashes}};
  napi_value r, v;
  NAPI_CALL(env, napi_create_object(env, &r));
  for (size_t k = 0; k < sizeof u / sizeof u[0]; k++) {
    NAPI_CALL(env, napi_create_uint32(env, u[k].val, &v));
    NAPI_CALL(env, napi_set_named_property(env, r, u[k].name, v));
  }
  return r;
}

static napi_value BitsPathStats(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value a[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, a, NULL, NULL));
  addon_ctx* c = get_ctx(env, a[0]);
  if (!c) return NULL;
  bgv_bits_path p;
  pthread_mutex_lock(&c->mu);
  const int st = bgv_bits_path_stats(c->ctx, &p);
  pthread_mutex_unlock(&c->mu);
  if (st != BGV_OK) return throw_bgv(env, st);
  napi_value r, v;
  NAPI_CALL(env, napi_create_object(env, &r));
  NAPI_CALL(env, napi_create_uint32(env, p.sets_complement, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "setsComplement", v));
  NAPI_CALL(env, napi_create_uint32(env, p.keys_expanded, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "keysExpanded", v));
  NAPI_CALL(env, napi_create_uint32(env, p.keys_gathered, &v));
  NAPI_CALL(env, napi_set_named_property(env, r, "keysGathered", v));
  return r;
}

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
