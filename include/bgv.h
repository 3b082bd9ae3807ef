/*
 * bgv.h -- C ABI of the MI355X (gfx950) BLS12-381 signature-set batch
 * verifier ("bgv" = BLS GPU verifier).
 *
 * This is the drop-in boundary for the hot path of
 *   IBlsVerifier.verifySignatureSets(sets, opts)
 *   (packages/beacon-node/src/chain/bls/interface.ts:20-51)
 * in maschad/lodestar.  Every entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no torch / HIP
 * types appear in the signatures.  All functions return 0 (BGV_OK) on
 * success or a negative BGV_E* status; per-set verification outcomes are
 * reported as the positive blst error codes listed in bgv_set_code.
 *
 * Threading: a bgv_ctx owns one HIP device and four streams.  Calls on one
 * context must be serialised by the caller (the N-API / Python host layers
 * do this); different contexts may be used from different threads.
 */
#ifndef BGV_H
#define BGV_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGV_ABI_VERSION 4

/* ---- status of an API call (negative) ---------------------------------- */
enum bgv_status {
  BGV_OK = 0,
  BGV_E_INVALID_ARG = -1,
  BGV_E_HIP = -2,          /* HIP runtime error (device missing, OOM, fault) */
  BGV_E_NO_DEVICE = -3,
  BGV_E_TABLE_RANGE = -4,  /* pubkey index outside the resident table */
  BGV_E_EMPTY_SET = -5,    /* a set with zero pubkeys (EMPTY_AGGREGATE_ARRAY) */
  BGV_E_BAD_PUBKEY = -6,   /* bgv_pubkeys_set: a key does not deserialize (the
                              text names the key and its BLST_* code) */
  BGV_E_STATE = -7,        /* bgv_partial_finish without a preceding bgv_partial */
};

/* ---- per-set / per-job outcome codes (>= 0) ------------------------------
 * Numbering follows blst's BLST_ERROR enum (the codes @chainsafe/blst turns
 * into "BLST_ERROR: BLST_<NAME>" exceptions), plus the size condition
 * @chainsafe/blst raises before reaching blst and a range guard for
 * device-resident index lists.                                             */
enum bgv_set_code {
  BGV_SET_OK = 0,
  BGV_SET_BAD_ENCODING = 1,
  BGV_SET_POINT_NOT_ON_CURVE = 2,
  BGV_SET_POINT_NOT_IN_GROUP = 3,
  BGV_SET_AGGR_TYPE_MISMATCH = 4,
  BGV_SET_VERIFY_FAIL = 5,
  BGV_SET_PK_IS_INFINITY = 6,
  BGV_SET_BAD_SCALAR = 7,
  BGV_SET_INVALID_SIZE = 8,
  BGV_SET_INDEX_RANGE = 9, /* device batch named a pubkey index >= table size */
};

/* job verdicts written to job_result[] */
enum bgv_job_result {
  BGV_JOB_INVALID = 0, /* encodings fine, pairing check failed -> resolve(false) */
  BGV_JOB_VALID = 1,   /* every set verified                  -> resolve(true)  */
  /* negative: -(bgv_set_code) of the first set (in set order) that could not
   * be parsed / validated -> reject(Error("BLST_ERROR: BLST_<NAME>"))       */
};

/* pubkey wire formats accepted by bgv_pubkeys_set */
enum bgv_pk_format {
  BGV_PK_COMPRESSED_48 = 0,   /* ZCash compressed G1, as in BeaconState.validators */
  BGV_PK_UNCOMPRESSED_96 = 1, /* x||y big-endian; PointFormat.uncompressed
                                 (multithread/index.ts:132,177) */
};

typedef struct bgv_ctx bgv_ctx;

/* One device batch = n_sets signature sets grouped into n_jobs jobs.  A job
 * is what the reference hands to verifySignatureSetsMaybeBatch
 * (chain/bls/maybeBatch.ts:16-38): its verdict is the AND of its sets.
 * Sets of one job are contiguous: job j owns sets [job_offsets[j],
 * job_offsets[j+1]).
 *
 * Pubkeys arrive as index lists into the HBM-resident index2pubkey table
 * (state-transition/src/cache/pubkeyCache.ts:6) instead of serialized
 * points: set i aggregates table entries pk_indices[pk_offsets[i] ..
 * pk_offsets[i+1]).  An index with bit 31 set selects entry
 * (index & 0x7fffffff) of raw_pks instead (pubkeys not in the table, e.g.
 * BLS-to-execution changes, signatureSets/blsToExecutionChange.ts:32).
 * An index past the table (or past n_raw) rejects only its job, with set
 * code BGV_SET_INDEX_RANGE: the reference fails such a lookup on the caller's
 * side (index2pubkey[i] is undefined), so other co-batched jobs are unaffected.
 * A set with no pubkeys fails the whole call with BGV_E_EMPTY_SET (callers
 * reject EMPTY_AGGREGATE_ARRAY before batching, chain/bls/utils.ts:11).
 * Host batches are copied into pinned staging memory first and every
 * contract check runs on that copy, so a caller that mutates its arrays
 * during the call cannot make the device read out of bounds.  On-device
 * batches (on_device = 1) are trusted to satisfy the contract: offsets
 * monotone, job_offsets spanning [0, n_sets], pk_indices as long as
 * pk_offsets[n_sets].
 *
 * Signatures: sig_len[i] bytes at sigs + 192*i (96 = compressed,
 * 192 = uncompressed; any other length yields BGV_SET_INVALID_SIZE, the
 * reference's "BLST_INVALID_SIZE", e2e/chain/bls/multithread.test.ts:97).
 *
 * scalars: 64-bit non-zero random multipliers, one per set (blst
 * mul_n_aggregate randomness).  NULL = drawn inside the library
 * (production): ChaCha20 on the device, keyed per call by 32 bytes of
 * getrandom().  Tests inject them for reproducibility.
 *
 * When `on_device` is non-zero every array pointer is a device pointer on
 * the context's device (inputs already resident in HBM); otherwise they are
 * host pointers and the library stages them.  The library works on its own
 * streams: every write to a device-resident input (and to an output buffer
 * such as bgv_gen_sign's sigs_out) must be complete before the call, e.g.
 * the producing stream synchronized (lodestar_amd/native.py does this for
 * torch tensors).                                                         */
typedef struct bgv_batch {
  uint32_t n_sets;
  uint32_t n_jobs;
  const uint32_t* job_offsets; /* [n_jobs + 1] */
  const uint32_t* pk_offsets;  /* [n_sets + 1] */
  const uint32_t* pk_indices;  /* [pk_offsets[n_sets]] */
  const uint8_t* raw_pks;      /* [n_raw][96] uncompressed big-endian, may be NULL */
  uint32_t n_raw;
  const uint8_t* msgs;         /* [n_sets][32] signing roots */
  const uint8_t* sigs;         /* [n_sets][192] */
  const uint32_t* sig_len;     /* [n_sets] */
  const uint64_t* scalars;     /* [n_sets] or NULL */
  uint32_t on_device;
} bgv_batch;

/* Timings of the last bgv_verify call (ms, HIP events around each stage on
 * the stream it ran on; stages 0-3 run concurrently on three streams, so their
 * times overlap and total_ms is less than their sum) plus the counters the reference pool exports as
 * lodestar_bls_thread_pool_* metrics (metrics/metrics/lodestar.ts:350-430). */
#define BGV_N_STAGES 16
typedef struct bgv_stats {
  float stage_ms[BGV_N_STAGES]; /* see bgv_stage_name() */
  float total_ms;
  uint32_t batch_retries;       /* 1 when the whole-batch check failed */
  uint32_t batch_sigs_success;  /* sets accepted by the whole-batch check */
  uint32_t n_sets;
  uint32_t n_jobs;
  uint64_t pubkeys_aggregated;  /* lodestar_bls_aggregated_pubkeys_total */
  /* the pipeline variant the batch ran with (chosen by batch size, or forced
   * by bgv_cfg); also filled by bgv_last_stats                              */
  uint32_t split;               /* 1: latency-mode hash and signature kernels */
  uint32_t miller_lanes;        /* set-pair Miller loop: lanes per pair (1 = one-lane loop) */
  uint32_t pairs_per_item;      /* one-lane loop: pairs sharing an accumulator */
  uint32_t msm;                 /* sum r_i sigma_i variant (bgv_cfg.msm) */
  uint32_t lines;               /* 1: fixed-argument Miller lines */
  uint32_t defer_from;          /* subgroup checks of sets >= defer_from run beside the Miller loops (n_sets: none) */
  uint32_t clear_lanes;         /* latency mode: lanes per point of the cofactor clearing */
  uint32_t miller_kv;           /* 0, or the product slots of the two-pair Miller loop in Karatsuba views (3 S lanes per two pairs) */
} bgv_stats;

/* Pipeline overrides for tests and A/B tools.  Production opens contexts with
 * bgv_open (every field "auto": the variant is chosen per batch by its size,
 * from measured sweeps).  No environment variable changes the pipeline.    */
typedef struct bgv_cfg {
  uint32_t struct_size; /* sizeof(bgv_cfg) */
  int32_t split;        /* -1 auto; 0 bulk kernels; 1 latency mode (two-lane hash maps, cooperative G2) */
  int32_t miller;       /* -1 auto; 1 one-lane set-pair loop; 2 / 4 two- / four-lane loop; 6 / 18 / 36 lanes per pair (cooperative) */
  int32_t job_lanes;    /* 0 auto (36); 6 / 18 / 36: lanes of the per-job (-G1, S_job) pairs */
  int32_t msm;          /* -1 auto; 0 per-set [r_i] sigma_i + tree; 1 per-job bucket MSM (one workgroup per job); 2 the (job, window)-lane MSM;
                           3 one-lane per-set [r_i] sigma_i + tree, subgroup checks deferred; 4 the (job, window, digit)-lane MSM */
  int32_t pairs;        /* 0 auto; 1 / 2 / 4 pairs per one-lane Miller work item (4: over precomputed lines only, else 2) */
  int32_t prefold;      /* -1 auto; 0 / 1 two-level per-job Miller fold */
  int32_t lines;        /* -1 auto; 0 / 1 fixed-argument lines (bulk mode, one-lane loop) */
  int32_t defer_pct;    /* -1 auto; 0..100: share of the G2 subgroup checks run beside the Miller loops (bulk mode) */
  int32_t timing;       /* -1 auto (batches >= 65,536 sets); 0 / 1 per-stage timing events */
  int32_t clear_lanes;  /* -1 auto; 1 / 3 / 9 lanes per point of the latency mode's cofactor clearing */
  int32_t miller_kv;    /* -1 auto; 0 off; 2 / 3 / 6 / 9: the two-pair Miller loop in Karatsuba views on 6 / 9 / 18 / 27 lanes per two pairs */
  int32_t cu_split;     /* 0: every CU of the device (default).  N > 0: a PRIORITY context whose streams run only
                           on N reserved CUs (the highest CU ids: with N = 8k, k CUs of every XCC), for
                           verifyOnMainThread single sets (multithread/index.ts:155-167) that must not wait for a
                           bulk batch's waves; N < 0: a bulk context whose streams leave those |N| CUs free (ABI 4) */
  int32_t miller_steps; /* -1 auto; 0 off; 1 on: the one-lane Miller stage over fixed-argument lines (split = 0, lines = 1)
                           as per-step line products: lanes (slice of a job's sets, line step) multiply the slice's 68
                           evaluated lines without any squaring, and one workgroup per job runs the squaring chain
                           once over the step products (bgv_miller_path_stats).  Auto turns
                           it on where the layout itself chose two pairs per item over lines (bgv_cfg.pairs and
                           bgv_cfg.lines left at auto); an explicit pairs keeps the item loop.  Results never depend
                           on it.  (hash_dedup stays the last field.) */
  int32_t hash_dedup;   /* -1 auto; 0 off; 1 on: a bulk-layout batch evaluates hash_to_G2 once per distinct signing
                           root and copies H(m) to the other sets that carry it (bgv_hash_stats).  Auto is OFF:
                           with every root distinct the grouping costs 2.3 ms per 100,352-set batch when three
                           batches are in flight (nothing alone), so a caller whose batches repeat roots opts in
                           (half of the roots repeated: 1.4 ms of 36.1 gained alone, 0.75 of 32.5 in flight; three
                           quarters: 4.5 and 3.4 ms).  Latency-mode batches (split = 1) hash every set whatever the
                           value.  Results never depend on it. */
} bgv_cfg;
/* every field "auto" */
void bgv_cfg_default(bgv_cfg* cfg);

int bgv_abi_version(void);
/* SHA-256 (hex) of the sources this library was compiled from (csrc + this
 * header, tools/build.py source_hash); bindings refuse a library whose id
 * differs from the tree beside it, so a stale build is never run */
const char* bgv_build_id(void);
const char* bgv_set_code_name(int code); /* "BLST_BAD_ENCODING", ... */
const char* bgv_stage_name(int stage);
const char* bgv_last_error(void);        /* thread-local text of the last failure */

/* Open a context on HIP device `device` (chain/chain.ts:199-202 picks the
 * verifier at node start; this is the GPU branch's constructor, replacing
 * `new BlsMultiThreadWorkerPool(opts, modules)`, multithread/index.ts:120). */
int bgv_open(int device, bgv_ctx** out);
/* bgv_open with pipeline overrides (tests, A/B tools); cfg may be NULL */
int bgv_open_cfg(int device, const bgv_cfg* cfg, bgv_ctx** out);
/* BlsMultiThreadWorkerPool.close (multithread/index.ts:193-214) */
int bgv_close(bgv_ctx* ctx);

/* index2pubkey table management: mirrors syncPubkeys / addPubkey
 * (state-transition/src/cache/pubkeyCache.ts:56-77, cache/epochContext.ts:
 * 701-704).  Keys are trusted (validated at deposit, block/processDeposit.ts:
 * 57-66) and stored as affine Montgomery (x, y), 96 B per validator.
 * Like PublicKey.fromBytes(pk, jacobian) (no validation) a key must still
 * deserialize: flags, x < p, on the curve; otherwise the call fails with
 * BGV_E_BAD_PUBKEY and the table is unchanged.  The infinity key is stored
 * as the identity (a set aggregating only identities is BLST_PK_IS_INFINITY).
 * The table is append-only like syncPubkeys: first_index <= current count
 * (rows below the count may be rewritten, as addPubkey does); a gap fails
 * with BGV_E_TABLE_RANGE.  At most 2^31 - 1 rows (bit 31 of an index
 * selects raw_pks).                                                       */
int bgv_pubkeys_set(bgv_ctx* ctx, uint32_t first_index, uint32_t n, const uint8_t* data, uint32_t format);
int bgv_pubkeys_count(bgv_ctx* ctx, uint32_t* count);
/* read back entries as 96-byte uncompressed big-endian (tests, checkpoints) */
int bgv_pubkeys_get(bgv_ctx* ctx, uint32_t first_index, uint32_t n, uint8_t* out96);

/* Untrusted-key validation: bls.PublicKey.fromBytes(pk, CoordType.affine,
 * validate=true) for n 48-byte compressed keys, as deposits do once per new
 * validator (state-transition/src/block/processDeposit.ts:57-66; also
 * beacon-node/src/chain/validation/blobsSidecar.ts:129).  codes[i] is a
 * bgv_set_code: 0 valid, BAD_ENCODING (flags / x >= p), POINT_NOT_ON_CURVE,
 * PK_IS_INFINITY, POINT_NOT_IN_GROUP ([r]P != O).  Valid keys can then be
 * appended with bgv_pubkeys_set.                                          */
int bgv_pubkeys_validate(bgv_ctx* ctx, const uint8_t* pk48, uint32_t n, int32_t* codes);

/* Verify one device batch.  Replaces the worker body
 * verifyManySignatureSets (multithread/worker.ts:30-106) together with
 * verifySignatureSetsMaybeBatch (maybeBatch.ts:16-38) and the main-thread
 * aggregation getAggregatedPubkey (chain/bls/utils.ts:5-16):
 *   job_result[n_jobs]  (host memory) BGV_JOB_* per job;
 *   set_code[n_sets]    (host memory, may be NULL) bgv_set_code per set;
 *   stats               (may be NULL).
 * One whole-batch pairing check runs first; only when it fails is every
 * job checked on its own (the worker's per-job retry, worker.ts:74-85). */
int bgv_verify(bgv_ctx* ctx, const bgv_batch* batch, int32_t* job_result, int32_t* set_code, bgv_stats* stats);
/* Stage timings (stage_ms, total_ms) of the last pipeline run on the context
 * (bgv_verify, bgv_partial, bgv_partial_finish); counters are left zero. */
int bgv_last_stats(bgv_ctx* ctx, bgv_stats* stats);

/* ---- same-message batches --------------------------------------------------
 * IBlsVerifier.verifySignatureSetsSameMessage (upstream Lodestar): gossip
 * attestations (chain/validation/attestation.ts:271) are single-pubkey sets,
 * and all members of a committee that vote for the same head sign the same
 * signing root.  For sets that share a message
 *   prod_i e(pk_i, H(m))^{r_i} = e(sum_i r_i pk_i, H(m)),
 * so a group of n sets needs n signature decodes and subgroup checks, one
 * weighted G1 sum over table rows, one weighted G2 sum, ONE hash and TWO
 * Miller pairs.  Additive to ABI 4: no existing entry point changes.
 *
 * Sets are grouped by message: group g owns sets [group_offsets[g],
 * group_offsets[g+1]) and msgs holds one root per GROUP.  Every set has
 * exactly one key: pk_indices[i] is a table row, or with bit 31 set a row of
 * raw_pks, as in bgv_batch.  Host batches are staged and checked like
 * bgv_batch (offsets monotone and spanning [0, n_sets], scalars non-zero);
 * an empty group, or n_groups > n_sets, is BGV_E_INVALID_ARG.  On-device
 * batches are trusted to satisfy the contract.  n_sets == 0 succeeds with no
 * output.
 *
 * The result is per set, because callers act per attestation:
 *  - A set is rejected before aggregation, with set_valid = 0 and its
 *    bgv_set_code, and left out of its group's sums when its signature does
 *    not decode or fails the subgroup check (codes as bgv_verify), is the
 *    identity (BGV_SET_VERIFY_FAIL), when its index is out of range
 *    (BGV_SET_INDEX_RANGE) or its key is the identity
 *    (BGV_SET_PK_IS_INFINITY).  One malformed signature does not force its
 *    neighbours into the retry.
 *  - Groups are cut into segments of at most 64 sets.  Per segment over the
 *    surviving sets P = sum r_i pk_i and S = sum r_i sigma_i; one whole-batch
 *    check prod ML(P, H(m_g)) ML(-G1, S) with one final exponentiation.  On
 *    success every surviving set is valid.
 *  - If it fails: one final exponentiation per segment, then every surviving
 *    set of a failing segment is decided on its own, e(pk_i, H(m_g))
 *    e(-G1, sigma_i) == 1, as a one-set job of the ordinary pipeline, inside
 *    the same call.  Such a set has set_valid = 0 and set_code 0 when it fails.
 *  - A segment whose P is the identity (e.g. a key beside its negation with
 *    equal scalars) is no error: its pair is skipped and its sets go to the
 *    per-set retry.
 * The call runs on the context's streams and counts as a batch in flight like
 * bgv_verify.                                                                */
typedef struct bgv_sm_batch {
  uint32_t n_sets;               /* single-pubkey sets */
  uint32_t n_groups;             /* distinct messages */
  const uint32_t* group_offsets; /* [n_groups + 1] */
  const uint32_t* pk_indices;    /* [n_sets]; bit 31 selects raw_pks */
  const uint8_t* raw_pks;        /* [n_raw][96], may be NULL */
  uint32_t n_raw;
  const uint8_t* msgs;           /* [n_groups][32] */
  const uint8_t* sigs;           /* [n_sets][192] */
  const uint32_t* sig_len;       /* [n_sets] */
  const uint64_t* scalars;       /* [n_sets] non-zero, or NULL = drawn on the device as bgv_verify does */
  uint32_t on_device;
} bgv_sm_batch;

/* counters that show which path ran */
typedef struct bgv_sm_stats {
  uint32_t n_sets, n_groups, n_segments;
  uint32_t hashes;         /* hash_to_G2 evaluations in the first pass */
  uint32_t pairs;          /* Miller pairs in the first pass */
  uint32_t groups_retried; /* groups with a segment that went to the per-set retry */
  uint32_t sets_retried;   /* sets decided on their own */
  float total_ms;          /* host clock around the call */
} bgv_sm_stats;

/* set_valid[n_sets] (host memory) 1 / 0 per set; set_code[n_sets] (host
 * memory, may be NULL) bgv_set_code of a rejected set, else 0; stats may be
 * NULL. */
int bgv_verify_same_message(bgv_ctx* ctx, const bgv_sm_batch* batch, uint8_t* set_valid, int32_t* set_code,
                            bgv_sm_stats* stats);
/* The host-side contract check of bgv_verify_same_message on its own (no
 * device, no context): BGV_OK or BGV_E_INVALID_ARG with bgv_last_error().
 * Offsets and scalars of an on-device batch are not read. */
int bgv_sm_check(const bgv_sm_batch* batch);
/* test-only: bgv_verify_same_message plus, per GROUP, P_g (96 B affine), S_g
 * (192 B affine) and H(m_g) (192 B affine) in the byte layout of bgv_debug,
 * all-zero for the identity.  Any output pointer may be NULL. */
int bgv_debug_same_message(bgv_ctx* ctx, const bgv_sm_batch* batch, uint8_t* set_valid, int32_t* set_code,
                           bgv_sm_stats* stats, uint8_t* p_group96, uint8_t* s_group192, uint8_t* h_group192);

/* ---- same-message verification that also returns each group's aggregate ----
 * In the reference a gossip attestation that verified goes straight into the
 * pre-aggregation pool, where the main thread decodes the same 96 bytes again
 * and adds the point to the committee's running aggregate:
 *   bls.Signature.aggregate([aggregate.signature, signatureFromBytesNoCheck(sig)])
 *   (chain/opPools/attestationPool.ts:182-199; :205-212 decodes the first
 *   attestation of a root; syncCommitteeMessagePool.ts:139 does the same for
 *   sync-committee messages).
 * That is one Fp2 square root and one G2 addition per attestation over exactly
 * the sets bgv_verify_same_message has just decoded, checked and grouped by
 * signing root (the pool's key, the AttestationData root, maps one to one to
 * the signing root within an epoch).  This entry returns, per group,
 *   agg_sig96[g] = compress(prev_g + sum of sigma_i over the group's sets with
 *                           set_valid = 1 and take != 0)
 * an UNWEIGHTED sum (the r_i-weighted sums of the pairing check are other
 * points), in the ZCash compressed form the pool stores.  Additive to ABI 4.
 *
 * set_valid, set_code and stats are exactly those of bgv_verify_same_message
 * on the same batch, whatever `agg` holds: they do not depend on take or prev.
 * A 192-byte (uncompressed) input signature is aggregated like a compressed
 * one; the output is always compressed.  take and prev_sig96 follow
 * batch->on_device: device pointers for a resident batch, otherwise staged
 * with the other arrays.  n_sets == 0 succeeds and writes nothing.
 *
 * Only the single-key entry has this form.  The aggregate-set entries
 * (bgv_verify_same_message_agg, _bits) feed aggregatedAttestationPool.ts:322,
 * which merges on disjoint bitfields: a different rule, not built here.
 *
 * The sums run on the pubkey stream beside the Miller, fold and final-
 * exponentiation stages, over the sets the classification left in; when a
 * segment goes to the per-set retry they run once more over the final
 * verdicts.
 * When it pays (one MI355X, host batches): the two sum
 * kernels take 0.57 ms of device time at 4,096 sets (64 groups of 64) and
 * 1.3 ms at 31,232 (64 groups of 488), most of it beside the pairing stages:
 * the clean call is 0.18 ms slower than bgv_verify_same_message at 4,096 sets
 * (8.77 -> 8.94 ms) and 0.24 ms at 31,232 (10.63 -> 10.87 ms).  That is more
 * than the plain call's run-to-run spread (0.015 / 0.022 ms): the sums are not
 * free, they cost 2 %.  With 1 % wrong-message signatures the retry dominates
 * both calls and the second pass adds 0.8 ms (22.6 -> 23.4 ms) and 1.4 ms
 * (71.1 -> 72.5 ms).  What the caller saves, one Fp2 square root and one G2
 * addition per attestation on its main thread, is not measured here.  A caller
 * that does not keep a pool of compressed aggregates gains nothing: use
 * bgv_verify_same_message. */
typedef struct bgv_sm_agg {
  const uint8_t* take;       /* [n_sets] or NULL (= every set): 0 keeps a set out of its group's aggregate;
                                it is verified and reported like any other (the pool's AlreadyKnown bit,
                                attestationPool.ts:190; two messages of one validator in one batch) */
  const uint8_t* prev_sig96; /* [n_groups][96] or NULL: the group's running aggregate, compressed; the
                                compressed identity (0xc0, 95 x 0) = none.  Trusted like
                                signatureFromBytesNoCheck: decoded, NOT subgroup-checked */
  uint8_t* agg_sig96;        /* out, host [n_groups][96]: compress(prev + sum of sigma_i over the sets with
                                set_valid = 1 and take != 0); the compressed identity when that is the identity */
  uint32_t* agg_count;       /* out, host [n_groups], may be NULL: sets added (prev not counted) */
  int32_t* agg_code;         /* out, host [n_groups], may be NULL: 0, or the bgv_set_code with which prev did
                                not decode (BAD_ENCODING, POINT_NOT_ON_CURVE); agg_sig96[g] is then the sum of
                                the new sets alone */
} bgv_sm_agg;
int bgv_verify_same_message_aggregate(bgv_ctx* ctx, const bgv_sm_batch* batch, const bgv_sm_agg* agg, uint8_t* set_valid,
                                      int32_t* set_code, bgv_sm_stats* stats);
/* bgv_sm_check plus: agg and agg->agg_sig96 are non-NULL (host only, no device, no context) */
int bgv_sm_agg_check(const bgv_sm_batch* batch, const bgv_sm_agg* agg);
/* Device time (ms, HIP events on the pubkey stream) of the two sum kernels in
 * the first pass of the last bgv_verify_same_message_aggregate on the context;
 * 0 when the last same-message call was another entry. */
int bgv_sm_agg_ms(bgv_ctx* ctx, float* ms);

/* ---- same-message batches of aggregate sets --------------------------------
 * The same identity holds when a set's key is an aggregate:
 *   prod_i e(PK_i, H(m))^{r_i} = e(sum_i r_i PK_i, H(m)),  PK_i = sum_j pk_ij.
 * Gossip beacon_aggregate_and_proof objects (chain/validation/
 * aggregateAndProof.ts:164-179: about 16 aggregates per committee and slot
 * sign one AttestationData root) and the attestations of a block
 * (state-transition signatureSets/indexedAttestation.ts:40-47: several
 * aggregates of one committee and data) are such sets.  A group pays its
 * per-set key aggregation, which bgv_verify pays too, plus one hash and two
 * Miller pairs per segment.  Additive to ABI 4.
 *
 * Set i owns keys pk_indices[pk_offsets[i] .. pk_offsets[i+1]) (table rows,
 * or rows of raw_pks with bit 31 set), as in bgv_batch; everything else is
 * bgv_sm_batch.  Host batches are staged and checked on the pinned copy:
 * pk_offsets monotone and spanning [0, total], group offsets as for
 * bgv_sm_batch, scalars non-zero; a set without keys fails the call with
 * BGV_E_EMPTY_SET, as bgv_verify does.  On-device batches are trusted;
 * offsets that run backwards there still cause no out-of-bounds access.
 *
 * Semantics are bgv_verify_same_message's (per-set verdicts, rejection before
 * aggregation, 64-set segments, whole-batch check, per-segment final
 * exponentiation, per-set retry inside the call, an identity P of a segment
 * goes to the retry), with the key codes of an aggregate:
 *  - any index past the table (or past n_raw): BGV_SET_INDEX_RANGE;
 *  - PK_i is the identity (all rows the identity, or a key beside its
 *    negation): BGV_SET_PK_IS_INFINITY;
 *  - identity rows inside a finite aggregate add nothing;
 *  - signature codes take precedence over key codes; an identity signature
 *    reports BGV_SET_VERIFY_FAIL.
 * A batch whose pk_offsets is 0, 1, 2, ... gives the verdicts, codes and group
 * sums of bgv_verify_same_message on the same arrays.  The retry verifies a
 * set against its aggregated key PK_i, as a one-set job of the ordinary
 * pipeline with PK_i as a raw key.
 * When it pays: the call is a longer chain of kernels
 * than bgv_verify's latency mode, so one slot's ~1,000 aggregates are faster
 * as one-set jobs of bgv_verify; a batch that fills the device (tens of
 * thousands of sets) is several times faster here.                            */
typedef struct bgv_sma_batch {
  uint32_t n_sets;               /* aggregate sets */
  uint32_t n_groups;             /* distinct messages */
  const uint32_t* group_offsets; /* [n_groups + 1] */
  const uint32_t* pk_offsets;    /* [n_sets + 1] */
  const uint32_t* pk_indices;    /* [pk_offsets[n_sets]]; bit 31 selects raw_pks */
  const uint8_t* raw_pks;        /* [n_raw][96], may be NULL */
  uint32_t n_raw;
  const uint8_t* msgs;           /* [n_groups][32] */
  const uint8_t* sigs;           /* [n_sets][192] */
  const uint32_t* sig_len;       /* [n_sets] */
  const uint64_t* scalars;       /* [n_sets] non-zero, or NULL = drawn on the device */
  uint32_t on_device;
} bgv_sma_batch;

/* Outputs as bgv_verify_same_message; bgv_sm_stats is reused (callers count the
 * aggregated keys from pk_offsets). */
int bgv_verify_same_message_agg(bgv_ctx* ctx, const bgv_sma_batch* batch, uint8_t* set_valid, int32_t* set_code,
                                bgv_sm_stats* stats);
/* The host-side contract check on its own (no device, no context): BGV_OK,
 * BGV_E_INVALID_ARG or BGV_E_EMPTY_SET with bgv_last_error().  Offsets and
 * scalars of an on-device batch are not read. */
int bgv_sma_check(const bgv_sma_batch* batch);
/* test-only: bgv_verify_same_message_agg plus, per SET, PK_i before weighting
 * (96 B affine, all-zero when the set's key was rejected) and the per-group
 * outputs of bgv_debug_same_message.  Any output pointer may be NULL. */
int bgv_debug_same_message_agg(bgv_ctx* ctx, const bgv_sma_batch* batch, uint8_t* set_valid, int32_t* set_code,
                               bgv_sm_stats* stats, uint8_t* pk_set96, uint8_t* p_group96, uint8_t* s_group192,
                               uint8_t* h_group192);

/* ---- committee bitfields over resident index lists --------------------------
 * The reference never holds attesters as index lists.  It holds a committee (a
 * slice of the epoch's shuffling, or the 512-member sync committee) and a
 * participation bitfield, and expands them on the main thread at every
 * producer: aggregationBits.intersectValues(committeeIndices)
 * (state-transition/src/cache/epochContext.ts:620-623,
 * block/processSyncCommittee.ts:89, chain/validation/aggregateAndProof.ts:129,
 * syncCommitteeContributionAndProof.ts:118).  Here the committees live in HBM
 * beside the index2pubkey table and a set says "list L, window [off, off +
 * len), these bits"; the device expands it.  Additive to ABI 4.
 *
 * Index lists are per context, like the table replica.  bgv_index_list_set
 * replaces list `list_id` (n == 0 drops it).  Entries are table rows: an entry
 * with bit 31 set fails with BGV_E_INVALID_ARG and leaves the list unchanged.
 * An entry at or past the current table count is allowed (the table is
 * append-only and may grow later); the range check stays per set, in the
 * gather.  The list being replaced is freed only after every stream of the
 * context has drained.                                                       */
#define BGV_MAX_INDEX_LISTS 8 /* previous/current/next shuffling, current/next sync committee, spare */
int bgv_index_list_set(bgv_ctx* ctx, uint32_t list_id, const uint32_t* indices /* host */, uint32_t n);
int bgv_index_list_len(bgv_ctx* ctx, uint32_t list_id, uint32_t* n);

/* The keys of set i:
 *  - src[i].list < BGV_MAX_INDEX_LISTS: L[off + j] for every j < len whose bit
 *    is set, in ascending j; bit j is (bits[bits_off + (j >> 3)] >> (j & 7)) & 1
 *    (the SSZ bit order).  bits_off is a byte offset of any alignment; two sets
 *    may point at the same bytes.
 *  - src[i].list == BGV_SRC_EXPLICIT: pk_indices[off .. off + len), all of
 *    them (bit 31 selects raw_pks); bits_off is ignored.  Randao, proposer and
 *    exit signatures and raw BLS-to-execution keys come this way.
 * job_result, set_code and stats are those of bgv_verify on the bgv_batch whose
 * pk_offsets / pk_indices are that expansion and whose other fields are equal.
 *
 * Host batches are staged into pinned memory and checked on that copy
 * (bgv_bits_check runs the same checks alone); every refusal names the set in
 * bgv_last_error().  BGV_E_INVALID_ARG: job offsets that break the bgv_batch
 * rules; a list id that names no list that is set; off + len (in 64 bits) past
 * the list, or past n_indices for an explicit set; bits_off + ceil(len / 8) >
 * bits_len; a non-zero padding bit above len in the last byte (intersectValues
 * throws on a length mismatch); a key total that does not fit 32 bits.
 * BGV_E_EMPTY_SET: a set with no bit set, or an explicit set with len == 0.
 * On-device batches are trusted, but cause no access outside the lists, bits,
 * pk_indices or the expansion: a source that fails the span checks expands to
 * the single index 0x7fffffff (past any table), so its job is rejected with
 * BGV_SET_INDEX_RANGE, and padding bits are masked off.
 *
 * When it pays (tools/bench_bits.py; host-resident
 * batches, one MI355X): the call stages 16 B per set and the bitfields instead
 * of 4 B per key.  At the C4 range-sync segment (100,352 sets, 12.98 M keys)
 * that is 26.1 MB instead of 75.2 MB and the call is about 1.6 ms faster than
 * bgv_verify on explicit lists (39.7 against 41.3 ms, beyond either path's
 * run-to-run spread; the expansion kernels take 0.18 ms).  At one epoch (3,136
 * sets) and at a 64-set gossip batch the two are within the baseline's spread:
 * there the gain is the index lists the caller no longer builds on its main
 * thread, not device time.                                                   */
#define BGV_SRC_EXPLICIT 0xffffffffu
typedef struct bgv_set_src { uint32_t list, off, len, bits_off; } bgv_set_src; /* 16 B per set */
typedef struct bgv_bits_batch {
  uint32_t n_sets, n_jobs;
  const uint32_t* job_offsets; /* [n_jobs + 1], as bgv_batch */
  const bgv_set_src* src;      /* [n_sets] */
  const uint8_t* bits;         /* all bitfields, byte-packed */
  uint32_t bits_len;
  const uint32_t* pk_indices;  /* keys of explicit sets; bit 31 selects raw_pks */
  uint32_t n_indices;
  const uint8_t* raw_pks;      /* [n_raw][96], may be NULL */
  uint32_t n_raw;
  const uint8_t* msgs;         /* [n_sets][32] */
  const uint8_t* sigs;         /* [n_sets][192] */
  const uint32_t* sig_len;     /* [n_sets] */
  const uint64_t* scalars;     /* [n_sets] or NULL, as bgv_batch */
  uint32_t on_device;
} bgv_bits_batch;
/* Outputs as bgv_verify.  Counts as a batch in flight like bgv_verify. */
int bgv_verify_bits(bgv_ctx* ctx, const bgv_bits_batch* batch, int32_t* job_result, int32_t* set_code, bgv_stats* stats);
/* The host-side contract check on its own (no device, no context), against the
 * lengths of the lists (0: not set).  The arrays of an on-device batch are not
 * read. */
int bgv_bits_check(const bgv_bits_batch* batch, const uint32_t* list_len /* [BGV_MAX_INDEX_LISTS] */);
/* test-only: the expansion alone; msgs, sigs, sig_len and scalars are not read.
 * Always the full expansion: resident sums (below) are ignored.
 * pk_offsets[n_sets + 1] and *total (host memory) are always written; the
 * indices are copied to pk_indices (host memory, cap entries) when total <= cap,
 * else the call fails with BGV_E_INVALID_ARG. */
int bgv_debug_bits_expand(bgv_ctx* ctx, const bgv_bits_batch* batch, uint32_t* pk_offsets /* [n_sets+1] */,
                          uint32_t* pk_indices, uint32_t cap, uint32_t* total);
/* Device time (ms, HIP events) of the expansion kernels of the last
 * bgv_verify_bits on a context that records stage timings (bgv_cfg.timing = 1,
 * or a batch of >= 65,536 sets); 0 otherwise. */
int bgv_bits_expand_ms(bgv_ctx* ctx, float* ms);

/* ---- key sums for bitfield sets: window sum minus absent members ------------
 * On mainnet nearly every bit of a committee's bitfield is set, so the gather of
 * bgv_verify_bits reads almost the whole window of the list.  With the prefix
 * sums of a list resident, S[k] = sum of table[L[j]] over j < k (k = 0 .. n),
 * a set's aggregate key is
 *     PK = S[off + len] - S[off] - sum of table[L[off + j]] over the ABSENT j,
 * two reads and one addition for the window plus one addition per absent
 * member.  Additive to ABI 4; nothing changes for a context that never asks.
 *
 * bgv_index_list_sums(ctx, id, 1) builds the n + 1 sums of list `id` on the
 * device from the table rows as they are now (once per epoch, when a shuffling
 * or a sync committee is installed); enable = 0 drops them.  Stored form:
 * Jacobian, 144 B per entry (a 2^20-entry list: 151 MB per context), so the
 * build needs no inversion.  BGV_E_INVALID_ARG for a list that is not set;
 * BGV_E_TABLE_RANGE when an entry is at or past the current table count (the
 * list stays usable without sums).  Identity rows add nothing; equal
 * neighbours, a row beside its negation and a prefix that is the identity are
 * all exact (complete addition throughout).
 * Sums are never stale: bgv_index_list_set on a list drops that list's sums;
 * a bgv_pubkeys_set or bgv_gen_keys that writes any row below the table count
 * (a rewrite) drops the sums of EVERY list; pure appends keep them (every entry
 * of a list with sums was below the count when they were built).  The caller
 * asks again.  A dropped buffer is freed only after every stream of the context
 * has drained.  Sums are per context, like the lists and the table.
 *
 * The rule (one function, bits_complement in csrc/bits_expand.h, shared by the
 * host check and the kernels): with pop the set bits inside len and absent =
 * len - pop, a list set takes the complement path iff its list has sums and
 * absent + 2 < pop (the 2: the window's two reads and one addition cost what
 * two gathered keys cost).  Explicit sets, sources that fail the span checks
 * and sets of lists without sums take the direct path as before.  A complement
 * set with no absent member gathers no key at all; BGV_E_EMPTY_SET stays a
 * rule on pop.  job_result, set_code and bgv_stats are those of the direct path
 * (pubkeys_aggregated stays the participating keys; an identity aggregate is
 * BGV_SET_PK_IS_INFINITY).  bgv_verify_same_message_bits (below) uses sums by the
 * same rule; the explicit-list same-message entries and bgv_partial do not.
 *
 * When it pays (tools/bench_bits_sums.py; one MI355X,
 * host-resident batches, a context with sums against one without in the same
 * process, alternating): at the C4 range-sync segment (100,352 sets) the gather
 * stage falls from 14.8 to 3.3 ms at 100% participation and from 15.1 to 4.2 ms
 * at 99%, where 1% of the participating keys are still read.  The pubkey chain
 * does not gate a lone batch, so the call gains less: 39.6 -> 37.9 ms at 100%,
 * 39.7 -> 39.1 ms at 99% and 39.2 -> 38.6 ms at 90%, each beyond both paths'
 * run-to-run spread, through a shorter hash kernel.  With three batches in
 * flight the 99% shape takes 31.6 instead of 36.2 ms per batch.  At 60% and 50%
 * participation, at one epoch (3,136 sets) and at a 64-set gossip batch the two
 * contexts are within the baseline's spread: no shape measured is slower.  The
 * build takes 9.2 ms for a 2^20-entry list and 2.2 ms for a 512-entry list.  Not
 * measured: on-device batches, the callers' side.                             */
int bgv_index_list_sums(bgv_ctx* ctx, uint32_t list_id, uint32_t enable);
int bgv_index_list_has_sums(bgv_ctx* ctx, uint32_t list_id, uint32_t* has);
/* Device time (ms, HIP events around the scan kernels) of the context's last
 * successful bgv_index_list_sums(.., 1); 0 before the first. */
int bgv_index_list_sums_ms(bgv_ctx* ctx, float* ms);
/* Path counters of the last bgv_verify_bits or bgv_verify_same_message_bits on
 * the context: sets on the complement path, participating keys (sum of pop and
 * explicit lengths) and the keys the gather read.  A caller of committee sets
 * no longer holds the index lists, so the bindings take the aggregated-key
 * count (lodestar_bls_aggregated_pubkeys_total) of a same-message call from
 * keys_expanded. */
typedef struct bgv_bits_path {
  uint32_t sets_complement, keys_expanded, keys_gathered;
} bgv_bits_path;
int bgv_bits_path_stats(bgv_ctx* ctx, bgv_bits_path* out);
/* hash_to_G2 evaluations of the last bgv_verify, bgv_verify_bits, bgv_partial
 * or bgv_debug_stages on the context.  A block's attestations are several
 * aggregates of one committee and data, and a slot's gossip aggregates sign
 * one AttestationData root about 16 to a committee: a bulk-layout batch
 * (bgv_stats.split == 0) of a context opened with bgv_cfg.hash_dedup = 1
 * therefore groups its sets by signing root on the device, hashes one set of
 * every group and copies H(m) to the rest.  The caller groups nothing and
 * every output is byte for byte what hashing each set gives.  sets: the
 * batch's sets; dedup: 1 when the grouping ran; hashes: the evaluations, i.e.
 * the distinct roots when dedup is 1, else sets.  The count comes home with
 * the call's results (no synchronise of its own).  The same-message entries
 * report their own bgv_sm_stats.hashes; after one of them this returns zeros. */
typedef struct bgv_hash_path {
  uint32_t sets, hashes, dedup;
} bgv_hash_path;
int bgv_hash_stats(bgv_ctx* ctx, bgv_hash_path* out);
/* The Miller stage of the last batch whose layout the context chose (bgv_verify,
 * bgv_verify_bits, bgv_partial, bgv_debug_stages): steps = 1 when it ran as
 * per-step line products (bgv_cfg.miller_steps), slice_sets the sets of a job
 * one lane multiplies per step (else the pairs per work item of the one-lane
 * loop, 0 for the multi-lane layouts), items the work items of the batch
 * (slices, or one-lane loop items; 0 for the multi-lane layouts).
 * bgv_stats.pairs_per_item keeps reporting the configured pairs on the steps
 * path.  Host-side values: no device call. */
typedef struct bgv_miller_path {
  uint32_t steps, slice_sets, items;
} bgv_miller_path;
int bgv_miller_path_stats(bgv_ctx* ctx, bgv_miller_path* out);
/* One Miller pair per distinct signing root of a job (opt-in, off by default;
 * DESIGN.md section 3i).  A job's verdict is the AND of its sets, and only the
 * job's product is ever read (the whole-batch check, the per-job retry,
 * bgv_partial), so with merging on the sets of a job that carry the same root
 * m pair once, as (sum_i r_i PK_i, H(m)) over the already scaled keys, where
 * they paired once each.  Classes never span jobs: the same root in two jobs
 * gives two pairs.  The caller groups nothing; job_result, set_code and every
 * bgv_stats counter are those of the unmerged run.  Signature decoding and
 * subgroup checks, the per-set gather and scaling, S_job and its (-G1, S_job)
 * pair, the folds, the final exponentiations and the per-job retry are
 * unchanged; the fixed-argument lines are computed and stored once per class.
 *
 * Where it applies: bgv_verify, bgv_verify_bits and bgv_partial (with
 * bgv_partial_finish) on a batch that runs the bulk layout (bgv_stats.split ==
 * 0) with the one-lane set-pair loop (bgv_stats.miller_lanes == 1): its item
 * loop at 1, 2 or 4 pairs per item, with or without lines, and the per-step
 * line products (bgv_cfg.miller_steps).  Every other layout (latency mode, the
 * two-, four- and many-lane loops) runs unmerged and reports merged = 0.  The
 * same-message entries already pay one pair per segment: they never merge and
 * leave zeros below.  bgv_debug_stages stays the per-set plan.  Merging implies
 * the root classes of bgv_cfg.hash_dedup for that batch, whatever the field
 * says (bgv_hash_stats reports dedup = 1).
 *
 * With merging on, bgv_partial's 576 bytes may differ from the unmerged bytes
 * (Miller values are not canonical: the product of two pairs' values and the
 * value of the summed pair differ by a factor the final exponentiation kills);
 * the verdict after bgv_combine_final does not.
 *
 * Fallback: a class whose keys sum to the identity (reachable only with
 * injected scalars, e.g. a key beside its negation with equal scalars) has the
 * pair value 1, which the item loop cannot tell from a rejected pair.  A device
 * flag comes home with the results the call copies anyway; when it is set the
 * call discards the pass, runs the batch again unmerged before it returns and
 * reports fallback = 1, merged = 0.  Results never depend on the switch.
 *
 * When it pays (one MI355X, the 100,352-set range-sync segment, 784 jobs of
 * 128, consecutive sets of a block sharing a root in runs of g;
 * tools/bench_pair_merge.py, profiles/pair_merge.json, DESIGN.md section 3i;
 * against hash_dedup = 0 / against hash_dedup = 1):
 *   g = 2 (half of the pairs merged)      lone 35.2 -> 30.5 ms (4.7 / 3.6 ms gained),
 *                                         three in flight 30.9 -> 26.2 ms per batch (4.7 / 4.2)
 *   g = 4 (three quarters merged)         lone 35.3 -> 26.4 ms (8.9 / 5.7),
 *                                         three in flight 30.8 -> 20.8 ms per batch (10.0 / 7.4)
 *   g = 1 (every root distinct)           lone inside the spread (35.1 against 35.2 ms); three in flight
 *                                         2.6 ms per batch SLOWER than hash_dedup = 0 (33.4 against 30.8),
 *                                         the cost hash_dedup = 1 has there too (33.4): the class set-up
 *                                         queues behind the other batches' waves
 * so a caller whose jobs repeat roots opts in, and one whose roots are all
 * distinct keeps it off.  The default stays off; there is no auto rule yet.
 *
 * mode: 0 off (default), 1 on; any other value BGV_E_INVALID_ARG.  Takes
 * effect from the next call on the context. */
int bgv_pair_merge(bgv_ctx* ctx, int32_t mode);
/* The set-pair part of the Miller stage of the last bgv_verify, bgv_verify_bits
 * or bgv_partial on the context: sets the batch's sets, pairs the set pairs it
 * ran (the classes when merged = 1, else sets), fallback 1 when a merged pass
 * was discarded.  Zeros after any other entry.  The class count comes home with
 * the call's results (no synchronise of its own). */
typedef struct bgv_pair_path {
  uint32_t sets, pairs, merged, fallback;
} bgv_pair_path;
int bgv_pair_stats(bgv_ctx* ctx, bgv_pair_path* out);
/* Batch-first tail of the steps path (additive to ABI 4).
 * A batch on the steps path (bgv_miller_path.steps) with the (job, window) MSM
 * gets its whole-batch verdict from ONE (-G1, sum_j S_job) pair and ONE Miller
 * recurrence over the step products of all its slices; the per-job signature
 * sums, (-G1, S_job) pairs and chains run behind that verdict, on the device
 * and with no host round trip, and only when it failed (the worker's per-job
 * retry).  Verdicts, set codes and bgv_stats are those of the per-job tail;
 * bgv_partial's 576 bytes differ as a field element and agree after the final
 * exponentiation.  mode: -1 auto (on wherever the steps path is; the default),
 * 0 off, 1 on (still only on that path).  From the next call on the context;
 * bgv_debug_stages and bgv_debug_pair_classes always run the per-job tail.
 * BGV_E_INVALID_ARG for a null context or any other mode. */
int bgv_batch_tail(bgv_ctx* ctx, int32_t mode);
/* The tail of the context's last bgv_verify / bgv_verify_bits / bgv_partial(+
 * _finish): batch_first 1 when it ran batch-first, retried 1 when its batch
 * check failed and the per-job kernels ran (always 0 right after bgv_partial:
 * the check is bgv_partial_finish's).  Zeros after bgv_debug_stages and
 * bgv_debug_pair_classes, which run the per-job tail. */
typedef struct bgv_tail_path {
  uint32_t batch_first, retried;
} bgv_tail_path;
int bgv_tail_stats(bgv_ctx* ctx, bgv_tail_path* out);
/* test-only: bgv_verify through the merged path (whatever bgv_pair_merge says;
 * BGV_E_STATE when the batch's layout does not merge) plus cls[n_sets] (class
 * index of every set), class_off[n_jobs + 1], p_class96[n_sets][96] (P_c affine
 * in bgv_debug's layout, all-zero for the identity or a rejected member; the
 * first class_off[n_jobs] rows), job_fe[n_jobs][576], batch_fe[576] (final
 * exponentiations of the job products and of the batch product, as
 * bgv_debug).  Any output may be NULL.  bgv_pair_stats reports the call. */
int bgv_debug_pair_classes(bgv_ctx* ctx, const bgv_batch* batch, int32_t* job_result, int32_t* set_code, uint32_t* cls,
                           uint32_t* class_off, uint8_t* p_class96, uint8_t* job_fe, uint8_t* batch_fe);
/* Host-only plan (no device, no context): bgv_bits_check's checks, then the
 * rule against list_has_sums[BGV_MAX_INDEX_LISTS] (NULL: no list has sums).
 * path[i] = 1 for a complement set (path may be NULL); *keys_gathered the keys
 * the gather would read.  The arrays of an on-device batch are not read (path
 * untouched, *keys_gathered = 0). */
int bgv_bits_plan(const bgv_bits_batch* batch, const uint32_t* list_len, const uint8_t* list_has_sums,
                  uint8_t* path /* [n_sets] or NULL */, uint64_t* keys_gathered);
/* test-only: the aggregate key of every set before scaling, through the
 * expansion, the rule and the gather of bgv_verify_bits: pk_agg96[n_sets][96] in
 * the layout of bgv_debug.pk_agg (all-zero for the identity or a rejected
 * key), path[n_sets], pk_code[n_sets] (0, BGV_SET_PK_IS_INFINITY or
 * BGV_SET_INDEX_RANGE).  msgs, sigs, sig_len and scalars are not read.  Any
 * output may be NULL. */
int bgv_debug_bits_keys(bgv_ctx* ctx, const bgv_bits_batch* batch, uint8_t* pk_agg96, uint8_t* path, int32_t* pk_code);
/* test-only: entries S[first .. first + n) of a list's sums as affine 96 B
 * (x || y big-endian), all-zero for the identity. */
int bgv_debug_index_list_sums(bgv_ctx* ctx, uint32_t list_id, uint32_t first, uint32_t n, uint8_t* out96);

/* ---- same-message batches of committee sets ----------------------------------
 * bgv_verify_same_message_agg for a caller that keeps its committees resident:
 * the aggregates of one committee and one AttestationData are windows of one
 * resident list with nearly every bit set, and the per-set key aggregation is
 * the one cost a same-message group still pays in full.  Groups are those of
 * bgv_sm_batch (one root per GROUP); the keys of set i are given exactly as in
 * bgv_bits_batch: a list window plus participation bits, or a BGV_SRC_EXPLICIT
 * run of pk_indices (bit 31 selects raw_pks).  Additive to ABI 4.
 *
 * The contract: set_valid, set_code and bgv_sm_stats (all but total_ms) are
 * those of bgv_verify_same_message_agg on the bgv_sma_batch whose pk_offsets /
 * pk_indices are the expansion of src and bits (bit order and expansion rule of
 * bgv_verify_bits) and whose other fields are equal, whether or not the context
 * holds sums: per-set verdicts, rejection before aggregation, 64-set segments,
 * the whole-batch check, the per-segment final exponentiation, the per-set
 * retry against PK_i as a raw key, an identity P of a segment going to the
 * retry, signature codes before key codes.  With sums resident a list set takes
 * the complement path by the rule of bgv_index_list_sums.
 *
 * Host batches are staged and checked on the pinned copy (bgv_smb_check runs
 * the same checks alone).  The group rules are bgv_sma_check's (offsets
 * monotone and spanning [0, n_sets], no empty group, n_groups <= n_sets,
 * scalars non-zero), the source rules bgv_bits_check's (the list is set, off +
 * len in 64 bits, bits_off + ceil(len / 8) <= bits_len, zero padding bits, a
 * key total that fits 32 bits); a set with no bit set, or an explicit set with
 * len == 0, is BGV_E_EMPTY_SET.  Every refusal names its set or group.
 * n_sets == 0 succeeds with no output.  On-device batches are trusted but
 * bounded as in bgv_verify_bits: a source that fails the span checks expands to
 * the single index 0x7fffffff, which here rejects only that set
 * (BGV_SET_INDEX_RANGE, set_valid = 0); padding bits are masked.
 *
 * When it pays: DESIGN.md section 3f, tools/bench_same_message_bits.py.        */
typedef struct bgv_smb_batch {
  uint32_t n_sets, n_groups;
  const uint32_t* group_offsets; /* [n_groups + 1], as bgv_sm_batch */
  const bgv_set_src* src;        /* [n_sets], as bgv_bits_batch */
  const uint8_t* bits;           /* all bitfields, byte-packed */
  uint32_t bits_len;
  const uint32_t* pk_indices;    /* keys of explicit sets; bit 31 selects raw_pks */
  uint32_t n_indices;
  const uint8_t* raw_pks;        /* [n_raw][96], may be NULL */
  uint32_t n_raw;
  const uint8_t* msgs;           /* [n_groups][32] */
  const uint8_t* sigs;           /* [n_sets][192] */
  const uint32_t* sig_len;       /* [n_sets] */
  const uint64_t* scalars;       /* [n_sets] non-zero, or NULL = drawn on the device */
  uint32_t on_device;
} bgv_smb_batch;
/* Outputs as bgv_verify_same_message_agg.  bgv_bits_path_stats reports the call. */
int bgv_verify_same_message_bits(bgv_ctx* ctx, const bgv_smb_batch* batch, uint8_t* set_valid, int32_t* set_code,
                                 bgv_sm_stats* stats);
/* The host-side contract check on its own (no device, no context), against the
 * lengths of the lists (0: not set).  The arrays of an on-device batch are not
 * read. */
int bgv_smb_check(const bgv_smb_batch* batch, const uint32_t* list_len /* [BGV_MAX_INDEX_LISTS] */);
/* test-only: the outputs of bgv_debug_same_message_agg plus path[n_sets]
 * (1 = complement path).  Any output pointer may be NULL. */
int bgv_debug_same_message_bits(bgv_ctx* ctx, const bgv_smb_batch* batch, uint8_t* set_valid, int32_t* set_code,
                                bgv_sm_stats* stats, uint8_t* pk_set96, uint8_t* path, uint8_t* p_group96,
                                uint8_t* s_group192, uint8_t* h_group192);

/* ---- same-message retry that localises failing sets by subset checks ---------
 * The retry of the four same-message entries (bgv_verify_same_message,
 * _aggregate, _agg, _bits) decides every surviving set of every failing segment
 * as a one-set job of the ordinary pipeline: the set is decoded, subgroup-
 * checked and hashed a second time, scaled, paired twice and gets a final
 * exponentiation of its own.  A remote peer controls how often that happens.
 *
 * bgv_sm_retry(ctx, 1) switches the context to the split retry.  It uses only
 * what the first pass left on the device (the decoded signatures, the keys and
 * H(m_g)), so it decodes and hashes nothing:
 *  - A retried segment's m surviving sets, in set order, are cut into subs: m
 *    subs of one set when m <= BGV_SM_SUB, else ceil(m / BGV_SM_SUB) subs of
 *    BGV_SM_SUB sets with a shorter last one (bgv_sm_split_plan).
 *  - Level 1: per sub P = sum r_i pk_i and S = sum r_i sigma_i with the batch's
 *    scalars, and the check e(P, H(m_g)) e(-G1, S) == 1, all subs of the call
 *    as one virtual batch.  A passing sub makes its sets valid; a failing sub
 *    of one set makes it invalid (the scaled check is the unscaled one raised
 *    to r_i != 0).  A sub whose P is the identity skips its pair and counts as
 *    failed, as a segment does.
 *  - Level 2: every set of a failing sub of two or more sets is a leaf,
 *    e(pk_i, H(m_g)) e(-G1, sigma_i) == 1 unscaled, all leaves as one virtual
 *    batch.  Leaf verdicts are exact.
 * set_valid, set_code, every field of bgv_sm_stats but total_ms and the
 * outputs of bgv_verify_same_message_aggregate are those of mode 0
 * (sets_retried stays "surviving sets of retried segments", pairs the first
 * pass's).  The one place where the modes can differ: a caller who injects
 * scalars chosen so that the faults of one sub cancel (sum r_i (sigma_i -
 * sk_i H(m)) = 0 over the sub) has that sub accepted where mode 0 would have
 * opened it, exactly as the faults of a whole segment can cancel in either
 * mode.  With the scalars the library draws this has probability 2^-64 per sub
 * check, the bound the whole-batch check rests on.
 *
 * When it pays (one MI355X, host batches, wrong-message
 * faults, mode 0 and mode 1 alternating on one context, p50 over three
 * repeats of 20 calls; mode 0's run-to-run spread is 0.01 to 0.17 ms):
 *   31,232 sets (64 groups of 488, one slot), 1 % faults: 71.3 -> 39.5 ms;
 *                                             0.1 % faults: 25.0 -> 24.3 ms;
 *   4,096 sets (64 groups of 64),             1 % faults: 22.8 -> 22.7 ms, level
 *                                             (inside the spread);
 *                                             0.1 % faults (4 bad sets):
 *                                             16.6 -> 22.1 ms, 5.5 ms SLOWER.
 * Clean calls are level at both shapes (8.7 and 10.6 ms): the first pass is
 * untouched.  Each level is a chain of lone-wave kernels that takes about
 * 6.7 ms however few subs it holds, so the mode pays where many segments fail
 * (a slot's worth of committees, many faults) and costs where a few sets of a
 * small batch do.  That is why it is opt-in and the default stays mode 0.
 * Not measured: batches in flight beside the call, on-device inputs, fault
 * rates above 1 %, the aggregate-set entries. */
/* mode: 0 per-set retry through the ordinary pipeline (default, as before),
 * 1 split retry; any other value or a null ctx: BGV_E_INVALID_ARG.  From the next call on. */
int bgv_sm_retry(bgv_ctx* ctx, int32_t mode);

typedef struct bgv_sm_retry_path {
  uint32_t mode;         /* the mode the last same-message call ran its retry in */
  uint32_t segments;     /* segments that went to the retry (failed, or P_seg the identity) */
  uint32_t subs;         /* subs formed */
  uint32_t subs_failed;  /* subs whose check failed or whose P_sub was the identity */
  uint32_t leaves;       /* sets decided by a check of their own after the sub level */
  uint32_t pairs;        /* Miller pairs of the retry */
  uint32_t hashes;       /* hash_to_G2 evaluations of the retry */
} bgv_sm_retry_path;
/* host-side values, no device call.  A mode 0 call reports subs = subs_failed = 0,
 * leaves = sets_retried, pairs = 2 sets_retried and hashes = sets_retried; a
 * mode 1 call 2 pairs per sub that was paired plus 2 per leaf, and hashes = 0. */
int bgv_sm_retry_stats(bgv_ctx* ctx, bgv_sm_retry_path* out);

#define BGV_SM_SUB 8
/* Host only (no device, no context): the subs of one retried segment.  m = its surviving sets;
 * writes the sub offsets into sub_off[] (cap entries) and returns the number of subs.  The
 * offsets are one more than the subs, the last one m.  When they do not fit cap entries (or
 * sub_off is NULL) nothing is written and the result is 0xffffffff. */
uint32_t bgv_sm_split_plan(uint32_t m, uint32_t* sub_off, uint32_t cap);

/* Multi-GPU partials: run the batch up to, but excluding, the
 * final exponentiation and return this shard's Miller product (576 B, 12
 * Fp coefficients of w^0..w^5, c0||c1 each, 48-byte big-endian) with the
 * per-set codes and per-job provisional results (job_result may be NULL):
 * -code for a job rejected by a parse / subgroup / pubkey error (final),
 * 1 for every other job (valid iff the node's combined check passes).
 * ok_out = 1 when no job was rejected.  The shard's intermediates stay on
 * the context for bgv_partial_finish until the next call on it. */
int bgv_partial(bgv_ctx* ctx, const bgv_batch* batch, uint8_t* miller576, int32_t* set_code, int32_t* job_result,
                int32_t* ok_out);
/* Localisation after a failed combined check (SURVEY §8e "Failure"): the
 * final exponentiation of THIS shard's product, then per-job final
 * exponentiations only if it fails (the worker's per-job retry,
 * multithread/worker.ts:74-85), on the intermediates bgv_partial left.
 * job_result[n_jobs] as for bgv_verify.  BGV_E_STATE when the previous call
 * on the context was not bgv_partial. */
int bgv_partial_finish(bgv_ctx* ctx, int32_t* job_result, bgv_stats* stats);
/* Combine n partial Miller products and run ONE final exponentiation:
 * *is_one = 1 iff the product maps to 1 in GT. */
int bgv_combine_final(bgv_ctx* ctx, const uint8_t* millers576, uint32_t n, int32_t* is_one);

/* ---- test-only: per-stage intermediates (SURVEY §8c golden plan) --------
 * Runs bgv_verify on the batch and copies out the canonical values of every
 * stage.  Points are affine, plain big-endian: G1 x || y (96 B), G2
 * x.c0 || x.c1 || y.c0 || y.c1 (192 B); the identity and rejected entries
 * are all-zero.  GT values are 576 B as for bgv_partial and are the cube of
 * the textbook final exponentiation f^((p^12 - 1)/r) (the hard-part chain
 * computes 3 (p^4 - p^2 + 1)/r).  Any pointer may be NULL.
 *   pair_fe[n_sets + n_jobs]: FE of every Miller value: set pairs first
 *   (with P = 2 or 4 pairs per Miller work item, bgv_stats.pairs_per_item,
 *   the item's first entry, job offset + P k, holds the item's product and
 *   the other P - 1 the identity), then each job's (-G1, S_job) pair. */
typedef struct bgv_debug {
  uint8_t* sig_aff;  /* [n_sets][192] decoded signature (zero: invalid / identity) */
  uint8_t* h_aff;    /* [n_sets][192] H(m_i) */
  uint8_t* pk_agg;   /* [n_sets][96]  aggregated pubkey before the batch scalar */
  uint8_t* rpk_aff;  /* [n_sets][96]  r_i * aggregated pubkey */
  uint8_t* s_aff;    /* [n_jobs][192] S_job = sum over the job of r_i sigma_i */
  uint8_t* pair_fe;  /* [n_sets + n_jobs][576] */
  uint8_t* job_fe;   /* [n_jobs][576] FE of the job's Miller product */
  uint8_t* batch_fe; /* [576] FE of the whole-batch product */
} bgv_debug;
int bgv_debug_stages(bgv_ctx* ctx, const bgv_batch* batch, int32_t* job_result, int32_t* set_code, bgv_debug* out);

/* ---- synthetic workload generation (bench / tests; not on the verify path) */
/* table[first .. first+n) := sk_i * G1 with sk_i = SHA256("bgv-sk" || LE64(seed)
 * || LE32(i)) mod r; keeps sk on the device for bgv_gen_sign. */
int bgv_gen_keys(bgv_ctx* ctx, uint32_t first_index, uint32_t n, uint64_t seed);
/* sigs96[i] = compress((sum_{j in set i} sk_j mod r) * H(msgs[i])).
 * Pointers follow batch->on_device; sigs_out is in the same space. */
int bgv_gen_sign(bgv_ctx* ctx, const bgv_batch* batch, uint8_t* sigs_out192);

/* ---- field self-test (tests only) ---------------------------------------- */
/* The device's modular add/sub primitives on n operand pairs: ab_in holds
 * a_i || b_i as 2 x 12 little-endian u32 limbs (each < p; add and sub mod p
 * are independent of the Montgomery form), out receives BGV_FP_OPS_N
 * elements of 12 limbs per pair: a+b, a-b, [a+b, 2b] (dual add), [a-b, b-a]
 * (dual sub), [a+b, a-b] (add/sub pair), [a+b, 2a] unreduced (dual lazy
 * add), -a, [a+b unreduced, b-a] (lazy add / sub pair).  Host pointers. */
#define BGV_FP_OPS_N 13
int bgv_debug_fp_ops(bgv_ctx* ctx, const uint32_t* ab_in, uint32_t n, uint32_t* out);
/* The signature decode of Signature.fromBytes(sig, affine, true) without its
 * subgroup check (tests only; maybeBatch.ts:23,36): sigs192[i] holds a 96-byte
 * compressed or 192-byte uncompressed encoding (sig_len[i]); out192[i] gets the
 * affine point as x.c0 || x.c1 || y.c0 || y.c1, 48 big-endian bytes each
 * (zero for the identity or a failed decode), codes[i] the BGV set code.
 * Host pointers. */
int bgv_debug_g2_decode(bgv_ctx* ctx, const uint8_t* sigs192, const uint32_t* sig_len, uint32_t n, uint8_t* out192,
                        int32_t* codes);

/* ---- microbenchmarks for the roofline ------------------------ */
/* Montgomery Fp-mul throughput: `lanes` independent chains of `iters`
 * products; returns device ms (HIP events). */
int bgv_bench_fpmul(bgv_ctx* ctx, uint32_t lanes, uint32_t iters, float* ms);
/* raw v_mad_u64_u32 throughput: lanes * iters * 8 dependent-free mads */
int bgv_bench_mad(bgv_ctx* ctx, uint32_t lanes, uint32_t iters, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* BGV_H */
