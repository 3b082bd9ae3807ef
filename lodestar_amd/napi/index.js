"use strict";
// IBlsVerifier (packages/beacon-node/src/chain/bls/interface.ts:20-51) over
// the N-API addon, in plain CommonJS so it runs on the Node in this image.
// The TypeScript class a maintainer adds (INTEGRATION.md section 4) has the
// same shape; this file is what the addon's tests drive.
//
// It keeps the pool contract of BlsMultiThreadWorkerPool
// (multithread/index.ts:120-431) with the GPU context in the role of the
// worker:
//  * every call is chunked into jobs of <= 128 sets (chunkifyMaximizeChunkSize);
//  * batchable jobs wait in a buffer flushed after 100 ms or as soon as more
//    than 32 signature sets are buffered (queueBlsWork, index.ts:262-291);
//  * non-batchable jobs are queued and started on the next macro task;
//  * an idle context takes every queued job (a GPU wants one large batch; the
//    CPU pool packs <= 128 sets per worker message), and the library's
//    whole-batch check with per-job fallback keeps the worker's verdicts;
//  * canAcceptWork() = context idle-capacity and queue bound (index.ts:143-149);
//  * close() rejects buffered and queued jobs with QueueError
//    QUEUE_ERROR_QUEUE_ABORTED (index.ts:193-214, util/queue/errors.ts);
//  * the lodestar_bls_thread_pool_* metrics (metrics/metrics/lodestar.ts:
//    350-430) are kept under their names in `metrics`.
//
// Sets: {type: "single" | "aggregate", pubkey | pubkeys, signingRoot
// (Uint8Array 32), signature (Uint8Array)}.  A pubkey is {index} (a row of
// the HBM index2pubkey table) or {raw: Uint8Array(96)} (uncompressed x||y).
const path = require("path");

// Every context's device batch runs on a libuv pool thread; contexts on
// different devices run concurrently only if the pool has a thread for each
// (default 4).  libuv reads UV_THREADPOOL_SIZE once, when the pool first
// starts: in a host that has already done fs / crypto work (Lodestar has) this
// default is ignored, so the launcher sets it before Node starts
// (INTEGRATION.md section 4) and the constructor warns when it is too small.
const UV_POOL_PRESET = process.env.UV_THREADPOOL_SIZE;
if (!UV_POOL_PRESET) process.env.UV_THREADPOOL_SIZE = "16";

const addon = require(path.join(__dirname, "bgv.node"));

// the library must be compiled from the sources beside it (tools/build.py
// embeds their SHA-256 as bgv_build_id; lodestar_amd/native.py source_hash
// is the same digest): a stale libbgv.so is refused instead of run
function sourceHash(root = path.join(__dirname, "..", "..")) {
  const fs = require("fs");
  const crypto = require("crypto");
  const csrc = path.join(root, "lodestar_amd", "csrc");
  const files = fs.readdirSync(csrc).filter((f) => f.endsWith(".h") || f.endsWith(".hip")).sort()
    .map((f) => "lodestar_amd/csrc/" + f).concat(["include/bgv.h"]);
  const h = crypto.createHash("sha256");
  for (const rel of files) {
    const data = fs.readFileSync(path.join(root, rel));
    const len = Buffer.alloc(8);
    len.writeUInt32LE(data.length % 0x100000000, 0);
    len.writeUInt32LE(Math.floor(data.length / 0x100000000), 4);
    h.update(Buffer.concat([Buffer.from(rel + "\0"), len, data]));
  }
  return h.digest("hex");
}

// an install that ships bgv.node + libbgv.so without the csrc tree cannot be
// compared: the check is skipped with a warning (INTEGRATION.md section 3)
function checkBuildId(id = addon.buildId()) {
  let want;
  try {
    want = sourceHash();
  } catch (e) {
    console.warn(`BlsGpuVerifier: libbgv.so build id not checked (sources not readable: ${e.message})`);
    return;
  }
  if (id !== want && !id.startsWith(want + "+")) {
    throw Error(`libbgv.so was built from other sources (id ${id.slice(0, 16)}, tree ${want.slice(0, 16)}): rebuild`);
  }
}
checkBuildId();

const MAX_SIGNATURE_SETS_PER_JOB = 128; // multithread/index.ts:39
const MAX_BUFFERED_SIGS = 32; // multithread/index.ts:48
const MAX_BUFFER_WAIT_MS = 100; // multithread/index.ts:57
const MAX_JOBS_CAN_ACCEPT_WORK = 512; // multithread/index.ts:62
const MAX_SETS_PER_DEVICE_BATCH = 1 << 17;
const now = () => Number(process.hrtime.bigint()) / 1e6;
// CUs of the first device kept for verifyOnMainThread (bgv_cfg.cu_split): the top 32 ids are one CU of every
// shader engine, and any reservation costs that device's bulk context ~13% at C4 and ~20% at the 8-GPU shard size
// (DESIGN.md §3), so the priority side takes 32 rather than 8.  The default reserves them only on a pool of two or
// more devices, where sharded batches give device 0 a RESERVED_CAP-weighted share; a one-device pool keeps the
// whole chip for its bulk batches unless priorityCus asks for the split.
const PRIORITY_CUS = 32;
const RESERVED_CAP = require("./reserved_cap.json").RESERVED_CAP; // dist.py RESERVED_CAP: bulk pace of a device with reserved CUs
// a device batch of at least this many sets (and >= 2 jobs) is split by job
// over the idle devices (partial Miller products, ONE combined final
// exponentiation); smaller batches run whole on one device while the other
// devices take the next batch (lodestar_amd/verifier.py SHARD_MIN_SETS)
const SHARD_MIN_SETS = 4096;
// device batches in flight per GPU, one context each: the next batches' hash,
// pubkey and decode kernels fill the SIMDs that a batch's one-wave Miller
// phase leaves idle (C4 36.7 -> 33.1 ms per batch with 3, C4/8 shards
// 9.65 -> 8.35 ms; profiles/r06b_overlap_sizes.txt, DESIGN.md §5)
const CONTEXTS_PER_DEVICE = 3;
// non-batchable jobs start once a macro task passes without a new job
// (bounded), so the per-block calls of a range-sync segment
// (verifyBlocksSignatures.ts:30-47, sleep(0) every 8 blocks) coalesce
const MAX_QUIET_WAITS = 8;
const RAW_BIT = 0x80000000;
const MAX_INDEX_LISTS = 8; // BGV_MAX_INDEX_LISTS
const SRC_EXPLICIT = 0xffffffff; // BGV_SRC_EXPLICIT
const POPCOUNT8 = Uint8Array.from({length: 256}, (_, v) => { let c = 0; for (let x = v; x; x >>= 1) c += x & 1; return c; });
// the G1 generator, 96-byte uncompressed, and the identity signature: the priority context's sizing job
const G1_GENERATOR_96 = Uint8Array.from(Buffer.from(
  "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb" +
  "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1", "hex"));
const IDENTITY_SIG_96 = (() => { const b = new Uint8Array(96); b[0] = 0xc0; return b; })();
const EMPTY_JOB = -10; // BGV internal code: a job without sets

class QueueError extends Error {
  // util/queue/errors.ts: LodestarError<{code: QueueErrorCode.QUEUE_ABORTED}>
  constructor(code = "QUEUE_ERROR_QUEUE_ABORTED") {
    super(code);
    this.type = {code};
    this.code = code;
  }
}

// multithread/utils.ts:4-19
function chunkifyMaximizeChunkSize(arr, minPerChunk) {
  const chunkCount = Math.floor(arr.length / minPerChunk);
  if (chunkCount <= 1) return [arr];
  const perChunk = Math.ceil(arr.length / chunkCount);
  const out = [];
  for (let i = 0; i < arr.length; i += perChunk) out.push(arr.slice(i, i + perChunk));
  return out;
}

// the bitfield-length refusal of a committee set, made by the caller-side checks and again by the encoders
function bitfieldLengthError(s) {
  return Error(`committee set: ${s.bits.length} bitfield bytes for ${s.committee.length} members`);
}

// the caller-side checks of one committee set ({committee: {list, offset, length}, bits, ...})
function checkCommitteeSet(s) {
  const c = s.committee;
  if (!c || !s.bits || !(c.list >= 0 && c.list < MAX_INDEX_LISTS)) throw Error("committee set without a committee, bits or a valid list id");
  if (!(c.offset >= 0) || !(c.length >= 0) || c.offset + c.length > 0xffffffff || s.bits.length !== ((c.length + 7) >> 3)) throw bitfieldLengthError(s);
  if (!s.bits.some((b) => b !== 0)) throw Error("EMPTY_AGGREGATE_ARRAY"); // intersectValues gives no index
}

// the caller-side checks of getAggregatedPubkey (chain/bls/utils.ts:5-16),
// made before queueing so a bad call cannot fail a batch it shares
function checkSets(sets) {
  for (const s of sets) {
    if (s.type === "committee") checkCommitteeSet(s);
    else {
      const pks = s.type === "single" ? [s.pubkey] : s.pubkeys;
      if (!pks || pks.length === 0 || pks.some((pk) => !pk)) throw Error("EMPTY_AGGREGATE_ARRAY");
      for (const pk of pks) if (pk.raw && pk.raw.length !== 96) throw Error("raw pubkeys must be 96-byte uncompressed");
    }
    if (!s.signingRoot || s.signingRoot.length !== 32) throw Error("signingRoot must be 32 bytes");
  }
}

// hash_to_G2 per device batch (bgv_hash_stats): the sets that needed H(m) and the evaluations the device made
// (fewer where a bulk-layout batch repeats signing roots).  Added on first use, so the metrics object keeps its
// shape until a batch reports them.
function recordHashes(m, sets, res) {
  if (typeof res.hashes !== "number") return;
  m.hashToG2Sets = (m.hashToG2Sets || 0) + sets;
  m.hashToG2Evaluated = (m.hashToG2Evaluated || 0) + res.hashes;
}

// Set pairs of the Miller stage per device batch (bgv_pair_stats): the sets that needed a pair and the pairs the
// device ran (fewer where a context with pairMerge met repeated signing roots inside a job).  Added on first use too.
function recordPairs(m, sets, res) {
  if (!Number.isFinite(res.millerPairs)) return;
  m.millerPairsSets = (m.millerPairsSets || 0) + sets;
  m.millerPairsEvaluated = (m.millerPairsEvaluated || 0) + res.millerPairs;
}

function aggregatedPubkeysCount(sets) {
  let n = 0;
  for (const s of sets) {
    if (s.type === "aggregate") n += s.pubkeys.length;
    else if (s.type === "committee") for (const b of s.bits) n += POPCOUNT8[b];
  }
  return n;
}

function hasCommitteeSets(jobs) {
  return jobs.some((j) => j.some((s) => s.type === "committee"));
}

// The one encoder behind the five encode* functions: the typed arrays of a bgv_*_batch (include/bgv.h) from a walk
// over the caller's sets.  The walk runs twice, first to count, then, over arrays allocated once, to fill: a 2^17-set
// batch allocates its arrays once instead of growing JS arrays of up to ~17M indices, which kept the main thread in
// the garbage collector.  outer names the offsets that close a job or a group; keys says how a set names its keys:
// "single" (one key per set), "offsets" (a run of pkIndices closed by pkOffsets) or "sources" (src: 4 words per set,
// list, off, len, bitsOff: an explicit run of pkIndices, or a list source over the byte-packed bitfields).
class BatchWriter {
  constructor(outer, keys) {
    this.outer = outer;
    this.keys = keys;
    this.filling = false;
    this.n = this.nOuter = this.nMsgs = this.nKeys = this.nRaw = this.nBits = 0;
    this.offsets = this.pkOffsets = this.src = this.bits = this.pkIndices = this.msgs = this.sigs = this.sigLen = this.rawPks = null;
  }

  allocate() {
    // zero sizes are padded to one entry, except the arrays only the "sources" layout measures by its own counts
    const some = (x) => Math.max(x, 1);
    const sources = this.keys === "sources";
    this.offsets = new Uint32Array(this.nOuter + 1);
    this.pkOffsets = this.keys === "offsets" ? new Uint32Array(this.n + 1) : null;
    this.src = sources ? new Uint32Array(4 * this.n) : null;
    this.bits = sources ? new Uint8Array(this.nBits) : null;
    this.pkIndices = new Uint32Array(sources ? this.nKeys : some(this.nKeys));
    this.msgs = new Uint8Array(some(this.nMsgs) * 32);
    this.sigs = new Uint8Array(some(this.n) * 192);
    this.sigLen = new Uint32Array(some(this.n));
    this.rawPks = new Uint8Array(some(this.nRaw) * 96);
    this.n = this.nOuter = this.nMsgs = this.nKeys = this.nRaw = this.nBits = 0;
    this.filling = true;
  }

  // the four src words of the current set
  source(list, off, len, bitsOff) {
    const src = this.src;
    const o = 4 * this.n;
    src[o] = list;
    src[o + 1] = off;
    src[o + 2] = len;
    src[o + 3] = bitsOff;
  }

  // one key of the current set: {index}, {raw}, or (numbers: the two publicKeys encoders only) a validator index
  key(pk, numbers) {
    const number = numbers && typeof pk === "number";
    const raw = !number && pk.raw;
    if (!this.filling) {
      this.nKeys++;
      if (raw) this.nRaw++;
    } else if (raw) {
      this.pkIndices[this.nKeys++] = (RAW_BIT | this.nRaw) >>> 0;
      this.rawPks.set(raw, 96 * this.nRaw++);
    } else {
      this.pkIndices[this.nKeys++] = (number ? pk : pk.index) >>> 0;
    }
  }

  // a set's run of keys
  run(pks, numbers) {
    if (pks.length === 0) throw Error("EMPTY_AGGREGATE_ARRAY"); // PublicKey.aggregate, utils.ts:11
    if (this.filling && this.src) this.source(SRC_EXPLICIT, this.nKeys, pks.length, 0);
    for (const pk of pks) this.key(pk, numbers);
  }

  // a set's committee source ({committee: {list, offset, length}, bits})
  committee(s) {
    if (this.filling) {
      const c = s.committee;
      if (s.bits.length !== ((c.length + 7) >> 3)) throw bitfieldLengthError(s);
      this.source(c.list, c.offset, c.length, this.nBits);
      this.bits.set(s.bits, this.nBits);
    }
    this.nBits += s.bits.length;
  }

  // the signing root of the set (jobs) or of the group
  message(root) {
    if (this.filling) this.msgs.set(root, 32 * this.nMsgs);
    this.nMsgs++;
  }

  // the set's signature closes the set; one of another size than 96 or 192 leaves its slot zero (sigLen tells)
  signature(sig) {
    if (this.filling) {
      this.sigLen[this.n] = sig.length;
      if (sig.length === 96 || sig.length === 192) this.sigs.set(sig, 192 * this.n);
      if (this.pkOffsets) this.pkOffsets[this.n + 1] = this.nKeys;
    }
    this.n++;
  }

  // closes the job or group
  close() {
    this.nOuter++;
    if (this.filling) this.offsets[this.nOuter] = this.n;
  }

  // the batch, its keys in the order of the bgv_*_batch fields
  batch() {
    const {pkOffsets, src, bits, pkIndices, msgs, sigs, sigLen, rawPks} = this;
    const head = {[this.outer]: this.offsets};
    if (pkOffsets) return {...head, pkOffsets, pkIndices, msgs, sigs, sigLen, rawPks};
    if (src) return {...head, src, bits, pkIndices, msgs, sigs, sigLen, rawPks};
    return {...head, pkIndices, msgs, sigs, sigLen, rawPks};
  }
}

function encodeBatch(outer, keys, walk) {
  const w = new BatchWriter(outer, keys);
  walk(w);
  w.allocate();
  walk(w);
  return w.batch();
}

// jobs (arrays of sets) -> the SoA batch of include/bgv.h bgv_batch ("offsets") or, where a batch holds committee
// sets ({type: "committee", committee: {list, offset, length}, bits, signingRoot, signature}), bgv_bits_batch ("sources")
function encodeJobSets(jobs, keys) {
  return encodeBatch("jobOffsets", keys, (w) => {
    for (const job of jobs) {
      for (const s of job) {
        if (keys === "sources" && s.type === "committee") w.committee(s);
        else w.run((s.type === "single" ? [s.pubkey] : s.pubkeys) || [], false);
        w.message(s.signingRoot);
        w.signature(s.signature);
      }
      w.close();
    }
  });
}
const encodeJobs = (jobs) => encodeJobSets(jobs, "offsets");
const encodeJobsBits = (jobs) => encodeJobSets(jobs, "sources");

// groups [{message, sets}] -> the arrays of a same-message batch; `set` names the keys of one set
function encodeGroups(groups, keys, set) {
  return encodeBatch("groupOffsets", keys, (w) => {
    for (const g of groups) {
      if (g.sets.length === 0) throw Error("Empty signature set");
      w.message(g.message);
      for (const s of g.sets) {
        set(w, s);
        w.signature(s.signature);
      }
      w.close();
    }
  });
}

// The routing rule of both classes: a device batch that holds a committee set
// goes through bgv_verify_bits; any other batch takes exactly the path it took before.
function verifyJobs(ctx, jobSets, sync = false) {
  if (hasCommitteeSets(jobSets)) return (sync ? addon.verifyBitsSync : addon.verifyBits)(ctx, encodeJobsBits(jobSets));
  return (sync ? addon.verifySync : addon.verify)(ctx, encodeJobs(jobSets));
}

// the caller-side checks of one verifySignatureSetsSameMessage call, as checkSets makes them
function checkSameMessage(sets, message) {
  if (!message || message.length !== 32) throw Error("signingRoot must be 32 bytes");
  for (const s of sets) {
    if (!s || !s.publicKey) throw Error("EMPTY_AGGREGATE_ARRAY");
    if (s.publicKey.raw && s.publicKey.raw.length !== 96) throw Error("raw pubkeys must be 96-byte uncompressed");
  }
}

// calls [{sets, message}] -> the groups of ONE device call: one group per
// call, calls whose messages are byte-equal share a group (first appearance
// order).  where[k] = [start, end) of call k in the flattened sets.  A call
// that asks for its aggregate (call.agg, verifyAndAggregateSameMessage) ALWAYS
// forms its own group, because the aggregate is per call; groupOf[k] is the
// group of call k.
function mergeSameMessage(calls) {
  const byMsg = new Map();
  const order = [];
  calls.forEach((c, k) => {
    const key = c.agg ? `#${k}` : Buffer.from(c.message).toString("hex");
    if (!byMsg.has(key)) { byMsg.set(key, {message: c.message, calls: []}); order.push(key); }
    byMsg.get(key).calls.push(k);
  });
  const groups = [];
  const where = new Array(calls.length);
  const groupOf = new Array(calls.length);
  let pos = 0;
  for (const key of order) {
    const g = byMsg.get(key);
    const sets = [];
    for (const k of g.calls) {
      where[k] = [pos, pos + calls[k].sets.length];
      groupOf[k] = groups.length;
      pos += calls[k].sets.length;
      for (const s of calls[k].sets) sets.push(s);
    }
    groups.push({message: g.message, sets});
  }
  return {groups, where, groupOf};
}

// the compressed identity of G2: "no running aggregate", and the aggregate of no signature
const G2_IDENTITY_96 = (() => { const b = new Uint8Array(96); b[0] = 0xc0; return b; })();

// the caller-side checks of verifyAndAggregateSameMessage's own options
function checkAggregateOpts(sets, opts) {
  if (opts.previous != null && opts.previous.length !== 96) throw Error("BLST_ERROR: BLST_INVALID_SIZE");
  if (opts.take != null && opts.take.length !== sets.length) throw Error("take must have one entry per set");
}

// take (one byte per set; a plain call adds nothing to an aggregate) and prevSigs
// (96 B per group) of a merged device call with at least one aggregate call
function encodeAggregateSide(calls, merged, n) {
  const take = new Uint8Array(Math.max(n, 1));
  const prevSigs = new Uint8Array(Math.max(merged.groups.length, 1) * 96);
  for (let g = 0; g < merged.groups.length; g++) prevSigs.set(G2_IDENTITY_96, 96 * g);
  calls.forEach((c, k) => {
    if (!c.agg) return;
    const [lo, hi] = merged.where[k];
    for (let i = lo; i < hi; i++) take[i] = c.agg.take == null || c.agg.take[i - lo] ? 1 : 0;
    if (c.agg.previous != null) prevSigs.set(c.agg.previous, 96 * merged.groupOf[k]);
  });
  return {take, prevSigs};
}

// one call's share of a verifySameMessageAggregate result: booleans for a plain
// call, {valid, aggregate, count} for an aggregate call, or the Error that
// rejects it alone (its `previous` did not decode)
function aggregateCallResult(addonRef, call, res, where, g) {
  const valid = toBooleans(res.valid, where[0], where[1]);
  if (!call.agg) return valid;
  if (res.aggCode[g] !== 0) return Error(`BLST_ERROR: ${addonRef.codeName(res.aggCode[g])}`);
  return {valid, aggregate: res.aggSigs.slice(96 * g, 96 * g + 96), count: res.aggCount[g]};
}

// groups [{message, sets: [{publicKey, signature}]}] -> the arrays of include/bgv.h bgv_sm_batch
function encodeSameMessage(groups) {
  return encodeGroups(groups, "single", (w, s) => w.key(s.publicKey, false));
}

// the caller-side checks of one verifyAggregateSetsSameMessage call: every set is
// {publicKeys: [{index} | {raw} | validator index, ...], signature} with at least one key,
// or a committee set {committee: {list, offset, length}, bits, signature} (the checks of checkSets)
function checkAggregateSameMessage(sets, message) {
  if (!message || message.length !== 32) throw Error("signingRoot must be 32 bytes");
  for (const s of sets) {
    if (s && s.committee) {
      checkCommitteeSet(s);
      continue;
    }
    if (!s || !s.publicKeys || s.publicKeys.length === 0) throw Error("EMPTY_AGGREGATE_ARRAY");
    for (const pk of s.publicKeys) {
      if (pk === null || pk === undefined) throw Error("EMPTY_AGGREGATE_ARRAY");
      if (typeof pk !== "number" && pk.raw && pk.raw.length !== 96) throw Error("raw pubkeys must be 96-byte uncompressed");
    }
  }
}

// groups [{message, sets: [{publicKeys, signature}]}] -> the arrays of include/bgv.h bgv_sma_batch
function encodeSameMessageAgg(groups) {
  return encodeGroups(groups, "offsets", (w, s) => w.run(s.publicKeys, true));
}

function hasCommitteeKeys(groups) {
  return groups.some((g) => g.sets.some((s) => !!s.committee));
}

// groups [{message, sets}] -> the arrays of include/bgv.h bgv_smb_batch: a committee set
// {committee: {list, offset, length}, bits, signature} becomes a list source over the
// byte-packed bitfields, a set {publicKeys, signature} a BGV_SRC_EXPLICIT run of pkIndices
function encodeSameMessageBits(groups) {
  return encodeGroups(groups, "sources", (w, s) => (s.committee ? w.committee(s) : w.run(s.publicKeys, true)));
}

// The routing rule of both classes for aggregate sets that sign one message: a call that holds a committee set goes
// through bgv_verify_same_message_bits (the key count comes from the device, after the call); any other call takes
// exactly the path it took before (the key count is the batch's, n sets, added before the call).  Returns the batch,
// the addon call, and the two additions to lodestar_bls_aggregated_pubkeys_total.
function routeAggregateSets(groups, n, sync = false) {
  const bits = hasCommitteeKeys(groups);
  const batch = bits ? encodeSameMessageBits(groups) : encodeSameMessageAgg(groups);
  const entry = (bits ? "verifySameMessageBits" : "verifySameMessageAgg") + (sync ? "Sync" : "");
  return {call: (ctx) => addon[entry](ctx, batch), keysBefore: bits ? 0 : batch.pkOffsets[n], keysAfter: (res) => (bits ? res.pubkeysAggregated : 0)};
}

// booleans of the verdicts valid[lo .. hi)
function toBooleans(valid, lo = 0, hi = valid.length) {
  return Array.from(valid.subarray(lo, hi), (v) => v === 1);
}

// verifyAndAggregateSameMessage's request, for both classes: the result of a call without sets, or the call to queue
function aggregateRequest(sets, message, opts) {
  checkAggregateOpts(sets, opts);
  const previous = opts.previous != null ? opts.previous : null;
  if (sets.length === 0) return {result: {valid: [], aggregate: Uint8Array.from(previous || G2_IDENTITY_96), count: 0}};
  checkSameMessage(sets, message);
  return {call: {sets, message, agg: {previous, take: opts.take != null ? opts.take : null}}};
}

// the batch of one verifySameMessageAggregate device call over merged calls with n sets
function encodeAggregateCalls(calls, merged, n) {
  return {...encodeSameMessage(merged.groups), ...encodeAggregateSide(calls, merged, n)};
}

// device work of a job in Montgomery Fp products (lodestar_amd/dist.py
// job_work, from tools/fpmul_counts.json): per set 13,790, per pubkey
// reference 11 (one G1 mixed addition of the gather)
const WORK_PER_SET = 13790;
const WORK_PER_PUBKEY = 11;
function jobWork(sets) {
  let refs = 0;
  for (const s of sets) refs += s.type === "single" ? 1 : s.pubkeys.length;
  return sets.length * WORK_PER_SET + refs * WORK_PER_PUBKEY;
}

// whole jobs to `world` shards, greedy by work (largest first, each to the
// least loaded shard), job order kept inside a shard (dist.py shard_jobs);
// caps: relative speed per shard (load compared as load / cap)
function shardJobs(weights, world, caps = null) {
  const shards = Array.from({length: world}, () => []);
  const load = new Array(world).fill(0);
  const cap = caps || new Array(world).fill(1);
  let floor = Infinity;
  for (const w of weights) if (w > 0 && w < floor) floor = w;
  if (floor === Infinity) floor = 1;
  const order = weights.map((s, j) => j).sort((a, b) => weights[b] - weights[a] || a - b);
  for (const j of order) {
    let r = 0;
    for (let k = 1; k < world; k++) if (load[k] / cap[k] < load[r] / cap[r]) r = k;
    shards[r].push(j);
    load[r] += Math.max(weights[j], floor);
  }
  return shards.map((s) => s.sort((a, b) => a - b));
}

function jobOutcome(r) {
  if (r === 1) return {ok: true, value: true};
  if (r === 0) return {ok: true, value: false};
  if (r === EMPTY_JOB) return {ok: false, error: Error("Empty signature set")}; // maybeBatch.ts:29-31
  return {ok: false, error: Error(`BLST_ERROR: ${addon.codeName(-r)}`)};
}

function newMetrics() {
  const hist = () => ({count: 0, sum: 0});
  return {
    lodestar_bls_aggregated_pubkeys_total: 0,
    lodestar_bls_thread_pool_time_seconds_sum: 0,
    lodestar_bls_thread_pool_success_jobs_signature_sets_count: 0,
    lodestar_bls_thread_pool_error_jobs_signature_sets_count: 0,
    lodestar_bls_thread_pool_queue_job_wait_time_seconds: hist(),
    lodestar_bls_thread_pool_queue_length: 0,
    lodestar_bls_thread_pool_workers_busy: 0,
    lodestar_bls_thread_pool_job_groups_started_total: 0,
    lodestar_bls_thread_pool_jobs_started_total: 0,
    lodestar_bls_thread_pool_sig_sets_started_total: 0,
    lodestar_bls_thread_pool_batch_retries_total: 0,
    lodestar_bls_thread_pool_batch_sigs_success_total: 0,
    lodestar_bls_thread_pool_latency_to_worker: hist(),
    lodestar_bls_thread_pool_latency_from_worker: hist(),
    lodestar_bls_worker_thread_time_per_sigset_seconds: hist(),
    // verifyOnMainThread calls (mainThreadDurationInThreadPool, multithread/index.ts:156-167)
    lodestar_bls_thread_pool_main_thread_time_seconds: hist(),
    // verifySignatureSetsSameMessage: sets sent to the device, and groups that went to the per-set retry
    lodestar_bls_thread_pool_same_message_sig_sets_started_total: 0,
    lodestar_bls_thread_pool_same_message_retries_total: 0,
    // the retry of the same-message calls (bgv_sm_retry_stats): subs a split retry formed, sets decided by a check of
    // their own, Miller pairs of the retry
    sm_retry_subs: 0,
    sm_retry_leaves: 0,
    sm_retry_pairs: 0,
    // verifyAndAggregateSameMessage: signatures added to the callers' aggregates
    lodestar_bls_thread_pool_same_message_aggregated_sigs_total: 0,
    // verifyAggregateSetsSameMessage: the same two counters for aggregate sets
    lodestar_bls_thread_pool_same_message_agg_sig_sets_started_total: 0,
    lodestar_bls_thread_pool_same_message_agg_retries_total: 0,
  };
}

function observe(h, v) {
  h.count++;
  h.sum += v;
}

// the retry of the context's last same-message call into the pool's counters (the caller still holds the context)
function recordSmRetry(m, ctx) {
  const p = addon.smRetryStats(ctx);
  m.sm_retry_subs += p.subs;
  m.sm_retry_leaves += p.leaves;
  m.sm_retry_pairs += p.pairs;
}

// The buffered queue of one family of same-message calls (the pool holds two: single-key sets and aggregate sets).
// Batchable calls wait in a buffer of their own under the pool's rule (100 ms, or more than MAX_BUFFERED_SIGS
// signatures waiting); whatever is queued goes out as ONE merged device call on one bulk context, one group per
// call, calls with byte-equal messages sharing a group.  `kind` gives what differs between the two:
//   started, retries: the names of the family's two counters in the pool's metrics
//   encode(jobs, merged, n) -> send: encodes the merged call; send(ctx, metrics) issues it and resolves the addon's result
//   countFirst: the device call is counted before it is encoded (else after)
//   share(job, k, res, merged, metrics): call k's share of the result, or the Error that rejects it alone
class SameMessageQueue {
  constructor(pool, kind) {
    this.pool = pool;
    this.kind = kind;
    this.jobs = [];
    this.buffered = null;
    this.running = false;
    this.deviceCalls = 0; // merged device calls issued (test hook)
    this.run = this.run.bind(this);
    this.flush = this.flush.bind(this);
  }

  queue(call, batchable) {
    return new Promise((resolve, reject) => {
      const job = {...call, resolve, reject};
      if (batchable) {
        if (!this.buffered) this.buffered = {jobs: [], sigCount: 0, timeout: setTimeout(this.flush, MAX_BUFFER_WAIT_MS)};
        this.buffered.jobs.push(job);
        this.buffered.sigCount += call.sets.length;
        if (this.buffered.sigCount > MAX_BUFFERED_SIGS) {
          clearTimeout(this.buffered.timeout);
          this.flush();
        }
      } else {
        this.jobs.push(job);
        setTimeout(this.run, 0);
      }
    });
  }

  flush() {
    if (this.buffered) {
      this.jobs.push(...this.buffered.jobs);
      this.buffered = null;
      setTimeout(this.run, 0);
    }
  }

  async run() {
    const pool = this.pool;
    if (pool.closed || this.running || this.jobs.length === 0) return;
    this.running = true;
    const jobs = [];
    let n = 0;
    while (this.jobs.length > 0 && (jobs.length === 0 || n + this.jobs[0].sets.length <= pool.maxSetsPerDeviceBatch)) {
      const j = this.jobs.shift();
      jobs.push(j);
      n += j.sets.length;
    }
    const m = pool.metrics;
    try {
      const merged = mergeSameMessage(jobs);
      const {best} = pool.idleContexts();
      let send = this.kind.countFirst ? null : this.kind.encode(jobs, merged, n);
      this.deviceCalls++;
      m[this.kind.started] += n;
      if (!send) send = this.kind.encode(jobs, merged, n);
      const ctx = pool.ctxs[best >= 0 ? best : 0];
      const res = await send(ctx, m);
      m[this.kind.retries] += res.groupsRetried;
      recordSmRetry(m, ctx);
      m.lodestar_bls_thread_pool_time_seconds_sum += (res.workerEndMs - res.workerStartMs) / 1000;
      jobs.forEach((job, k) => {
        const r = this.kind.share(job, k, res, merged, m);
        if (r instanceof Error) job.reject(r);
        else job.resolve(r);
      });
    } catch (e) {
      for (const job of jobs) job.reject(e);
    }
    this.running = false;
    if (this.jobs.length > 0) setTimeout(this.run, 0);
  }

  // calls and sets waiting, for canAcceptWork
  waiting() {
    let sets = this.buffered ? this.buffered.sigCount : 0;
    for (const j of this.jobs) sets += j.sets.length;
    return {jobs: this.jobs.length + (this.buffered ? this.buffered.jobs.length : 0), sets};
  }

  // rejects what is buffered and queued (the pool is closing)
  abort() {
    if (this.buffered) {
      clearTimeout(this.buffered.timeout);
      for (const job of this.buffered.jobs) job.reject(new QueueError());
      this.buffered = null;
    }
    for (const job of this.jobs) job.reject(new QueueError());
    this.jobs = [];
  }
}

// verifySignatureSetsSameMessage and verifyAndAggregateSameMessage (bgv_verify_same_message, or
// bgv_verify_same_message_aggregate once a queued call asks for its aggregate)
const SINGLE_KEY_SETS = {
  started: "lodestar_bls_thread_pool_same_message_sig_sets_started_total",
  retries: "lodestar_bls_thread_pool_same_message_retries_total",
  countFirst: true,
  encode(jobs, merged, n) {
    if (jobs.some((j) => j.agg)) {
      const batch = encodeAggregateCalls(jobs, merged, n);
      return (ctx) => addon.verifySameMessageAggregate(ctx, batch);
    }
    const batch = encodeSameMessage(merged.groups);
    return (ctx) => addon.verifySameMessage(ctx, batch);
  },
  share(job, k, res, merged, m) {
    const r = aggregateCallResult(addon, job, res, merged.where[k], merged.groupOf[k]);
    if (job.agg && !(r instanceof Error)) m.lodestar_bls_thread_pool_same_message_aggregated_sigs_total += r.count;
    return r;
  },
};

// verifyAggregateSetsSameMessage (bgv_verify_same_message_agg, or bgv_verify_same_message_bits: routeAggregateSets)
const AGGREGATE_SETS = {
  started: "lodestar_bls_thread_pool_same_message_agg_sig_sets_started_total",
  retries: "lodestar_bls_thread_pool_same_message_agg_retries_total",
  countFirst: false,
  encode(jobs, merged, n) {
    const route = routeAggregateSets(merged.groups, n);
    return async (ctx, m) => {
      m.lodestar_bls_aggregated_pubkeys_total += route.keysBefore;
      const res = await route.call(ctx);
      m.lodestar_bls_aggregated_pubkeys_total += route.keysAfter(res);
      return res;
    };
  },
  share: (job, k, res, merged) => toBooleans(res.valid, merged.where[k][0], merged.where[k][1]),
};

class BlsGpuVerifier {
  // devices: HIP device ordinals, one context each, all owned by this process
  // (chain/chain.ts:199-202 constructs one verifier per node); every context
  // holds a replica of the pubkey table
  // priorityCus: CUs of the first device reserved for verifyOnMainThread
  // (bgv_cfg.cu_split, a multiple of 8): a priority context runs there, the
  // bulk context of that device leaves them free (~13-20% of its throughput
  // whatever the count: the shader engines that lost a CU set the pace;
  // sharded batches give that device a RESERVED_CAP-weighted shard).  Default:
  // PRIORITY_CUS on a pool of two or more devices, 0 on one device (the
  // priority context then shares every CU)
  // blsVerifyAllMultiThread (chain/options.ts:14, multithread/index.ts:124): verifyOnMainThread
  // calls join the pool's queue like any other; no CUs are then reserved and
  // no priority context is opened
  // contextsPerDevice: device batches in flight per GPU (one context each,
  // each with its own table replica); a batch large enough to shard is split
  // over one idle context per device
  // pairMerge (bgv_pair_merge, off by default): every bulk context pairs once per distinct signing root of a job
  // where its batch runs the bulk layout's one-lane loop; the priority context serves latency batches
  // smRetry (bgv_sm_retry, off by default): every context localises the failing sets of a same-message call by
  // subset checks (subs of 8, then the sets of the failing subs) instead of one-set jobs
  constructor({device = 0, devices = null, maxSetsPerDeviceBatch = MAX_SETS_PER_DEVICE_BATCH, shardMinSets = SHARD_MIN_SETS,
    priorityCus = null, blsVerifyAllMultiThread = false, contextsPerDevice = CONTEXTS_PER_DEVICE, pairMerge = false,
    smRetry = false} = {}) {
    const ids = devices && devices.length ? devices : [device];
    if (!(contextsPerDevice >= 1)) throw new Error(`contextsPerDevice ${contextsPerDevice}`);
    if (priorityCus === null || priorityCus === undefined) priorityCus = ids.length > 1 ? PRIORITY_CUS : 0;
    if (blsVerifyAllMultiThread) priorityCus = 0;
    this.blsVerifyAllMultiThread = blsVerifyAllMultiThread;
    // every device batch holds a libuv pool thread (napi_async_work); the pool
    // size is read once, when the pool first starts, so the launcher must set
    // UV_THREADPOOL_SIZE before Node runs any async work (INTEGRATION.md 4)
    // UV_THREADPOOL_SIZE; judged on the value the process started with: the
    // 16 this module assigns when it was unset only counts if the pool had
    // not started yet, which the module cannot tell, so it assumes libuv's 4
    const pool = Number(UV_POOL_PRESET) || 4;
    const nCtx = ids.length * contextsPerDevice;
    if (nCtx + 2 > pool) {
      const was = UV_POOL_PRESET ? `UV_THREADPOOL_SIZE=${pool}` : "UV_THREADPOOL_SIZE unset at start (libuv default 4)";
      console.warn(`BlsGpuVerifier: ${nCtx} device contexts with ${was}: device batches may ` +
        "serialise and starve other pool work; start Node with UV_THREADPOOL_SIZE >= contexts + 2");
    }
    // context k runs on device entry ctxDev[k]; every bulk context of the first
    // device leaves the reserved CUs free (one unmasked context would put bulk
    // waves on them)
    this.ctxDev = [];
    this.ctxs = [];
    ids.forEach((d, i) => {
      for (let c = 0; c < contextsPerDevice; c++) {
        this.ctxs.push(addon.open(d, i === 0 && priorityCus > 0 ? -priorityCus : 0));
        this.ctxDev.push(i);
      }
    });
    this.pairMerge = !!pairMerge;
    if (this.pairMerge) for (const c of this.ctxs) addon.pairMerge(c, true);
    this.nDevices = ids.length;
    this.contextsPerDevice = contextsPerDevice;
    this.ctx = this.ctxs[0];
    // verifyOnMainThread's own context (with its own table replica and mutex):
    // it never waits for a bulk batch's context lock or, with priorityCus, its
    // waves.  Under blsVerifyAllMultiThread nothing uses it: the blocking
    // verifySignatureSetsSync then runs on the first bulk context
    this.prio = blsVerifyAllMultiThread ? null : addon.open(ids[0], priorityCus > 0 ? priorityCus : 0);
    this.smRetry = !!smRetry;
    if (this.smRetry) for (const c of this.prio ? [...this.ctxs, this.prio] : this.ctxs) addon.smRetry(c, 1);
    this.prioReserved = priorityCus > 0;
    this.priorityCus = priorityCus;
    if (this.prio) this.warmPriority();
    this.prioBusy = 0;
    this.idle = this.ctxs.map(() => true);
    this.maxSetsPerDeviceBatch = maxSetsPerDeviceBatch;
    this.shardMinSets = shardMinSets;
    this.jobs = [];
    this.queuedSets = 0;
    this.bufferedJobs = null;
    this.busy = 0; // device batches in flight
    this.closed = false;
    this.runScheduled = false;
    this.pushSeq = 0;
    this.seenSeq = 0;
    this.quietWaits = 0;
    this.metrics = newMetrics();
    this.runJob = this.runJob.bind(this);
    this.runBufferedJobs = this.runBufferedJobs.bind(this);
    // verifySignatureSetsSameMessage and verifyAggregateSetsSameMessage: a queue and a buffer of their own each
    this.sm = new SameMessageQueue(this, SINGLE_KEY_SETS);
    this.sma = new SameMessageQueue(this, AGGREGATE_SETS);
    this.runSameMessage = this.sm.run;
    this.flushSameMessage = this.sm.flush;
    this.runSameMessageAgg = this.sma.run;
    this.flushSameMessageAgg = this.sma.flush;
  }

  // merged device calls issued per family (test hooks)
  get smDeviceCalls() { return this.sm.deviceCalls; }
  get smaDeviceCalls() { return this.sma.deviceCalls; }

  // syncPubkeys / addPubkey (pubkeyCache.ts:56-77): 48-byte compressed keys, every replica
  syncPubkeys(firstIndex, pubkeys48) {
    this.pubkeysSet(firstIndex, pubkeys48, 0);
  }

  // rows in either format (0: 48-byte compressed, 1: 96-byte uncompressed) into every replica
  pubkeysSet(firstIndex, bytes, format) {
    for (const c of this.allContexts()) addon.pubkeysSet(c, firstIndex, bytes, format);
  }

  // A resident index list (an epoch's shuffling, a sync committee) into every
  // context, like the pubkey table (bgv_index_list_set); an empty array drops
  // it.  Committee sets name it by committee.list.  Each context's call waits
  // for that context's batch in flight.  {sums: true} also builds the list's
  // resident prefix sums (bgv_index_list_sums): nearly full committees are then
  // taken as window sum minus absent members.  Every entry must be a row the
  // table already holds; a later pubkeysSet that rewrites a row drops the sums.
  setIndexList(id, indices, opts = {}) {
    for (const c of this.allContexts()) {
      addon.setIndexList(c, id, indices);
      if (opts.sums && indices.length) addon.setIndexListSums(c, id, true);
    }
  }

  // sizes the priority context's work buffers for a full job (128 sets) at
  // construction, so a verifyOnMainThread call never frees and regrows them
  // (a hipFree synchronises the device: it would wait for the bulk contexts'
  // batches in flight).  One dummy job: the generator as a raw key and the
  // identity signature; its verdict is ignored.
  warmPriority() {
    const set = {type: "single", pubkey: {raw: G1_GENERATOR_96}, signingRoot: new Uint8Array(32), signature: IDENTITY_SIG_96};
    addon.verifySync(this.prio, encodeJobs([new Array(MAX_SIGNATURE_SETS_PER_JOB).fill(set)]));
  }

  allContexts() {
    return this.prio ? this.ctxs.concat([this.prio]) : this.ctxs.slice();
  }

  // multithread/index.ts:143-149.  A queued job joins the next device batch,
  // so work is accepted while fewer than MAX_JOBS_CAN_ACCEPT_WORK jobs and
  // less than one full device batch of sets are queued, batch in flight or
  // not (gating on idle devices would stop the network processor,
  // network/processor/index.ts:406, for every 5-40 ms device batch)
  canAcceptWork() {
    const sm = this.sm.waiting();
    const sma = this.sma.waiting();
    return !this.closed && this.jobs.length + sm.jobs + sma.jobs < MAX_JOBS_CAN_ACCEPT_WORK &&
      this.queuedSets + sm.sets + sma.sets < this.maxSetsPerDeviceBatch;
  }

  // IBlsVerifier.verifySignatureSetsSameMessage (upstream Lodestar; the call
  // site is gossip attestation validation, chain/validation/attestation.ts:271):
  // sets = [{publicKey: {index} | {raw}, signature}] that all sign `message`;
  // resolves one boolean per set.  Batchable calls wait in a buffer of their
  // own under the pool's rule (100 ms, or more than 32 signatures waiting);
  // whatever is queued goes out as ONE merged device call
  // (bgv_verify_same_message) on one bulk context, one group per call, calls
  // with byte-equal messages sharing a group.
  async verifySignatureSetsSameMessage(sets, message, opts = {}) {
    if (this.closed) throw new QueueError();
    if (sets.length === 0) return [];
    checkSameMessage(sets, message);
    return this.sm.queue({sets, message, addedTimeMs: Date.now()}, opts.batchable);
  }

  // verifySignatureSetsSameMessage that also returns what the caller's
  // pre-aggregation pool would compute next (chain/opPools/attestationPool.ts:182-199,
  // syncCommitteeMessagePool.ts:139): resolves {valid: boolean[], aggregate:
  // Uint8Array(96), count} with aggregate = compress(previous + the signatures of
  // the valid sets whose `take` entry is true).  opts = {batchable, previous?:
  // Uint8Array(96), take?: boolean[]}.  The call rides the queue and buffer of
  // verifySignatureSetsSameMessage and always forms its own group of the merged
  // device call (bgv_verify_same_message_aggregate).  A `previous` that does not
  // decode rejects this call alone with BLST_ERROR: BLST_<NAME>.
  async verifyAndAggregateSameMessage(sets, message, opts = {}) {
    if (this.closed) throw new QueueError();
    const r = aggregateRequest(sets, message, opts);
    return r.result || this.sm.queue({...r.call, addedTimeMs: Date.now()}, opts.batchable);
  }

  // verifySignatureSetsSameMessage for aggregate sets (the aggregates of gossip
  // beacon_aggregate_and_proof objects, chain/validation/aggregateAndProof.ts:164-179,
  // or of one block's attestations for one committee and data):
  // sets = [{publicKeys: [{index} | {raw} | validator index, ...], signature}] that all
  // sign `message`; resolves one boolean per set, false for a rejected set.
  // Batchable calls wait in a buffer of their own, apart from the single-key
  // one, under the same rule, and go out as ONE merged device call
  // (bgv_verify_same_message_agg), one group per call.
  async verifyAggregateSetsSameMessage(sets, message, opts = {}) {
    if (this.closed) throw new QueueError();
    if (sets.length === 0) return [];
    checkAggregateSameMessage(sets, message);
    return this.sma.queue({sets, message, addedTimeMs: Date.now()}, opts.batchable);
  }

  async verifySignatureSets(sets, opts = {}) {
    if (this.closed) throw new QueueError();
    checkSets(sets);
    this.metrics.lodestar_bls_aggregated_pubkeys_total += aggregatedPubkeysCount(sets);
    if (opts.verifyOnMainThread && !this.blsVerifyAllMultiThread) return this.verifyPriority(sets);
    const results = await Promise.all(
      chunkifyMaximizeChunkSize(sets, MAX_SIGNATURE_SETS_PER_JOB).map((chunk) => this.queueBlsWork(chunk, opts))
    );
    if (results.length === 0) throw Error("Empty results array");
    return results.every((r) => r === true);
  }

  // verifyOnMainThread (multithread/index.ts:155-167; chain/validation/block.ts:146
  // for a gossip block's proposer signature): high priority and unbuffered, as
  // the reference runs it at once on the main thread, but without blocking the
  // event loop: one device batch on the priority context, on the libuv pool.
  // It bypasses the buffer, the job queue and the bulk contexts' locks.
  async verifyPriority(sets) {
    this.prioBusy++;
    const t0 = now();
    try {
      const bits = hasCommitteeSets([sets]);
      const batch = bits ? encodeJobsBits([sets]) : encodeJobs([sets]);
      const t1 = now();
      const pending = bits ? addon.verifyBits(this.prio, batch) : addon.verify(this.prio, batch);
      this.lastPriorityIssue = {encodeMs: t1 - t0, queueMs: now() - t1};
      const res = await pending;
      this.recordWork([{sets}], res);
      const o = jobOutcome(res.results[0]);
      if (!o.ok) throw o.error;
      return o.value;
    } finally {
      // timed in a finally like the reference's mainThreadDurationInThreadPool
      // (multithread/index.ts:156-167): calls that throw are observed too
      observe(this.metrics.lodestar_bls_thread_pool_main_thread_time_seconds, (now() - t0) / 1e3);
      this.prioBusy--;
    }
  }

  // BlsSingleThreadVerifier.verifySignatureSets (singleThread.ts:14-35):
  // maybeBatch on the calling thread, for callers that want exactly that;
  // the pool's verifyOnMainThread uses verifyPriority instead
  verifySignatureSetsSync(sets) {
    if (this.closed) throw new QueueError();
    checkSets(sets);
    const res = verifyJobs(this.prio || this.ctx, [sets], true);
    this.recordWork([{sets}], res);
    const o = jobOutcome(res.results[0]);
    if (!o.ok) throw o.error;
    return o.value;
  }

  // multithread/index.ts:255-292
  queueBlsWork(sets, opts) {
    if (this.closed) return Promise.reject(new QueueError());
    return new Promise((resolve, reject) => {
      const job = {resolve, reject, addedTimeMs: Date.now(), sets};
      if (opts.batchable) {
        if (!this.bufferedJobs) {
          this.bufferedJobs = {jobs: [], sigCount: 0, timeout: setTimeout(this.runBufferedJobs, MAX_BUFFER_WAIT_MS)};
        }
        this.bufferedJobs.jobs.push(job);
        this.bufferedJobs.sigCount += sets.length;
        if (this.bufferedJobs.sigCount > MAX_BUFFERED_SIGS) {
          clearTimeout(this.bufferedJobs.timeout);
          this.runBufferedJobs();
        }
      } else {
        this.pushJobs([job]);
        this.pushSeq++;
        this.scheduleRun();
      }
    });
  }

  pushJobs(jobs) {
    for (const j of jobs) this.queuedSets += j.sets.length;
    this.jobs.push(...jobs);
  }

  // the first look comes a macro task later, as in the reference
  // (setTimeout(runJob, 0), multithread/index.ts:242,299); the quiet-window
  // re-looks use setImmediate, which Node does not clamp to 1 ms, so a lone
  // block-import job pays microseconds for the coalescing, not milliseconds
  scheduleRun(quiet = false) {
    if (!this.runScheduled) {
      this.runScheduled = true;
      if (quiet) setImmediate(this.runJob);
      else setTimeout(this.runJob, 0);
    }
  }

  // multithread/index.ts:425-431 (the buffer has already waited: no quiet window)
  runBufferedJobs() {
    if (this.bufferedJobs) {
      this.pushJobs(this.bufferedJobs.jobs);
      this.bufferedJobs = null;
      this.scheduleRun();
    }
  }

  // every queued job up to maxSetsPerDeviceBatch sets
  prepareWork() {
    const jobs = [];
    let totalSigs = 0;
    while (this.jobs.length > 0 && (jobs.length === 0 || totalSigs + this.jobs[0].sets.length <= this.maxSetsPerDeviceBatch)) {
      const job = this.jobs.shift();
      jobs.push(job);
      totalSigs += job.sets.length;
    }
    this.queuedSets -= totalSigs;
    return jobs;
  }

  // idle contexts: the first idle one of each device (spread, for sharding)
  // and the idle one on the least busy device (for a whole batch)
  idleContexts() {
    const busyOn = new Array(this.nDevices).fill(0);
    this.idle.forEach((f, k) => { if (!f) busyOn[this.ctxDev[k]]++; });
    const spread = [];
    const seen = new Set();
    let best = -1;
    this.idle.forEach((f, k) => {
      if (!f) return;
      const dv = this.ctxDev[k];
      if (!seen.has(dv)) { seen.add(dv); spread.push(k); }
      if (best < 0 || busyOn[dv] < busyOn[this.ctxDev[best]]) best = k;
    });
    return {spread, best};
  }

  // multithread/index.ts:297-391: every idle context takes a device batch; a
  // batch of >= shardMinSets sets is split over one idle context per device
  runJob() {
    this.runScheduled = false;
    while (!this.closed && this.jobs.length > 0) {
      const {spread: idle, best} = this.idleContexts();
      if (idle.length === 0) return; // a finishing batch reschedules
      if (this.pushSeq !== this.seenSeq && this.quietWaits < MAX_QUIET_WAITS) {
        // jobs arrived since the last look: wait one more macro task
        this.seenSeq = this.pushSeq;
        this.quietWaits++;
        this.scheduleRun(true);
        return;
      }
      this.quietWaits = 0;
      this.seenSeq = this.pushSeq;
      const jobs = this.prepareWork();
      let n = 0;
      for (const j of jobs) n += j.sets.length;
      const devs = idle.length > 1 && jobs.length > 1 && n >= this.shardMinSets ? idle : [best];
      for (const k of devs) this.idle[k] = false;
      this.runDeviceBatch(jobs, devs);
    }
  }

  async runDeviceBatch(jobs, devs) {
    this.busy++;
    this.peakBusy = Math.max(this.peakBusy || 0, this.busy); // device batches in flight at once (test hook)
    const m = this.metrics;
    try {
      const now = Date.now();
      let started = 0;
      for (const job of jobs) {
        observe(m.lodestar_bls_thread_pool_queue_job_wait_time_seconds, (now - job.addedTimeMs) / 1000);
        started += job.sets.length;
      }
      m.lodestar_bls_thread_pool_job_groups_started_total += 1;
      m.lodestar_bls_thread_pool_jobs_started_total += jobs.length;
      m.lodestar_bls_thread_pool_sig_sets_started_total += started;
      // bgv_partial takes no bitfields: a batch with a committee set goes whole to one context
      const jobSets = jobs.map((j) => j.sets);
      const res = devs.length === 1 || hasCommitteeSets(jobSets)
        ? await verifyJobs(this.ctxs[devs[0]], jobSets)
        : await this.verifySharded(jobSets, devs);
      this.recordWork(jobs, res);
      jobs.forEach((job, k) => {
        const o = jobOutcome(res.results[k]);
        if (o.ok) job.resolve(o.value);
        else job.reject(o.error);
      });
    } catch (e) {
      for (const job of jobs) job.reject(e);
    }
    this.busy--;
    for (const k of devs) this.idle[k] = true;
    this.scheduleRun();
  }

  // SURVEY 8e: jobs sharded by work (sets + pubkey references) over the devices, one partial Miller
  // product per shard (bgv_partial, concurrently on the libuv pool), ONE final
  // exponentiation of their product (bgv_combine_final); only when it fails
  // does each shard localise its failing jobs (bgv_partial_finish, the
  // worker's per-job retry).  Returns the result shape of addon.verify.
  async verifySharded(jobSets, devs) {
    // the first device's bulk context leaves CUs to the priority context and
    // runs at RESERVED_CAP of the others' pace (dist.py)
    const caps = devs.map((k) => (this.ctxDev[k] === 0 && this.prioReserved ? RESERVED_CAP : 1));
    const shards = shardJobs(jobSets.map(jobWork), devs.length, caps);
    const live = [];
    shards.forEach((ids, r) => ids.length && live.push({ctx: this.ctxs[devs[r]], ids}));
    if (live.length === 1) return addon.verify(live[0].ctx, encodeJobs(jobSets));
    const parts = await Promise.all(live.map((s) => addon.partial(s.ctx, encodeJobs(s.ids.map((k) => jobSets[k])))));
    const millers = new Uint8Array(576 * live.length);
    parts.forEach((p, k) => millers.set(p.miller, 576 * k));
    const valid = await addon.combineFinal(live[0].ctx, millers);
    // a verifyOnMainThread call that ran on a context in between replaced its
    // pending partial (bgv error -7): that shard is verified again from scratch
    const finals = valid ? parts : await Promise.all(live.map((s) => addon.partialFinish(s.ctx).catch((e) => {
      if (!/bgv error -7/.test(e.message)) throw e;
      return addon.verify(s.ctx, encodeJobs(s.ids.map((k) => jobSets[k])));
    })));
    const results = new Int32Array(jobSets.length);
    let sigsOk = 0;
    live.forEach((s, k) => s.ids.forEach((j, i) => {
      results[j] = finals[k].results[i];
      if (valid && results[j] === 1) sigsOk += jobSets[j].length;
    }));
    return {
      results, batchRetries: valid ? 0 : 1, batchSigsSuccess: sigsOk,
      pubkeysAggregated: parts.reduce((a, p) => a + p.pubkeysAggregated, 0),
      hashes: parts.reduce((a, p) => a + p.hashes, 0), // per shard: a root on two shards is hashed on both
      millerPairs: parts.reduce((a, p) => a + p.millerPairs, 0),
      deviceMs: Math.max(...parts.map((p) => p.deviceMs)),
      workerStartMs: Math.min(...parts.map((p) => p.workerStartMs)),
      workerEndMs: Math.max(...finals.map((p) => p.workerEndMs)),
      shards: live.length,
    };
  }

  recordWork(jobs, res) {
    const m = this.metrics;
    let ok = 0;
    let err = 0;
    jobs.forEach((job, k) => {
      if (res.results[k] >= 0) ok += job.sets.length;
      else err += job.sets.length;
    });
    const workerSec = (res.workerEndMs - res.workerStartMs) / 1000;
    m.lodestar_bls_thread_pool_time_seconds_sum += workerSec;
    if (ok + err > 0) observe(m.lodestar_bls_worker_thread_time_per_sigset_seconds, workerSec / (ok + err));
    m.lodestar_bls_thread_pool_success_jobs_signature_sets_count += ok;
    m.lodestar_bls_thread_pool_error_jobs_signature_sets_count += err;
    m.lodestar_bls_thread_pool_batch_retries_total += res.batchRetries;
    m.lodestar_bls_thread_pool_batch_sigs_success_total += res.batchSigsSuccess;
    recordHashes(m, ok + err, res);
    recordPairs(m, ok + err, res);
  }

  // gauges sampled at scrape time (index.ts:135-139)
  metricsSnapshot() {
    this.metrics.lodestar_bls_thread_pool_queue_length = this.jobs.length;
    this.metrics.lodestar_bls_thread_pool_workers_busy = this.idle.filter((f) => !f).length;
    return this.metrics;
  }

  // multithread/index.ts:193-214
  async close() {
    if (this.closed) return;
    this.closed = true;
    if (this.bufferedJobs) {
      clearTimeout(this.bufferedJobs.timeout);
      for (const job of this.bufferedJobs.jobs) job.reject(new QueueError());
      this.bufferedJobs = null;
    }
    for (const job of this.jobs) job.reject(new QueueError());
    this.jobs = [];
    this.queuedSets = 0;
    this.sm.abort();
    this.sma.abort();
    for (const c of this.allContexts()) addon.close(c); // each waits for its batch in flight (the context mutex)
  }
}

// BlsSingleThreadVerifier (chain/bls/singleThread.ts:7-46), which chain.ts:200-202
// builds instead of the pool when blsVerifyAllMainThread is set: maybeBatch on
// one device context, blocking the calling thread as blst does on the main
// thread (addon.verifySync); canAcceptWork is always true.  Its pubkey table
// is its own replica.
class BlsGpuSingleThreadVerifier {
  constructor({device = 0, pairMerge = false, smRetry = false} = {}) {
    this.ctx = addon.open(device, 0);
    if (smRetry) addon.smRetry(this.ctx, 1); // bgv_sm_retry: the split retry of the same-message entries
    if (pairMerge) addon.pairMerge(this.ctx, true); // bgv_pair_merge: bulk-layout batches only
    this.closed = false;
    this.metrics = {lodestar_bls_aggregated_pubkeys_total: 0, lodestar_bls_thread_pool_main_thread_time_seconds: {count: 0, sum: 0}};
  }

  syncPubkeys(firstIndex, pubkeys48) {
    addon.pubkeysSet(this.ctx, firstIndex, pubkeys48, 0);
  }

  pubkeysSet(firstIndex, bytes, format) {
    addon.pubkeysSet(this.ctx, firstIndex, bytes, format);
  }

  setIndexList(id, indices, opts = {}) {
    addon.setIndexList(this.ctx, id, indices);
    if (opts.sums && indices.length) addon.setIndexListSums(this.ctx, id, true);
  }

  async verifySignatureSets(sets) {
    if (this.closed) throw new QueueError();
    this.metrics.lodestar_bls_aggregated_pubkeys_total += aggregatedPubkeysCount(sets);
    checkSets(sets); // getAggregatedPubkey's checks (utils.ts:5-16)
    const t0 = now();
    const res = verifyJobs(this.ctx, [sets], true);
    const o = jobOutcome(res.results[0]);
    if (!o.ok) throw o.error; // only runs without exceptions are timed, as in the reference
    observe(this.metrics.lodestar_bls_thread_pool_main_thread_time_seconds, (now() - t0) / 1e3);
    return o.value;
  }

  // verifySignatureSetsSameMessage on the calling thread: one device call, one group
  async verifySignatureSetsSameMessage(sets, message) {
    if (this.closed) throw new QueueError();
    if (sets.length === 0) return [];
    checkSameMessage(sets, message);
    return toBooleans(addon.verifySameMessageSync(this.ctx, encodeSameMessage([{message, sets}])).valid);
  }

  // verifyAndAggregateSameMessage on the calling thread: one device call, one group
  async verifyAndAggregateSameMessage(sets, message, opts = {}) {
    if (this.closed) throw new QueueError();
    const {result, call} = aggregateRequest(sets, message, opts);
    if (result) return result;
    const merged = mergeSameMessage([call]);
    const res = addon.verifySameMessageAggregateSync(this.ctx, encodeAggregateCalls([call], merged, sets.length));
    const r = aggregateCallResult(addon, call, res, merged.where[0], 0);
    if (r instanceof Error) throw r;
    return r;
  }

  // verifyAggregateSetsSameMessage on the calling thread: one device call, one group
  async verifyAggregateSetsSameMessage(sets, message) {
    if (this.closed) throw new QueueError();
    if (sets.length === 0) return [];
    checkAggregateSameMessage(sets, message);
    const route = routeAggregateSets([{message, sets}], sets.length, true);
    this.metrics.lodestar_bls_aggregated_pubkeys_total += route.keysBefore;
    const res = route.call(this.ctx);
    this.metrics.lodestar_bls_aggregated_pubkeys_total += route.keysAfter(res);
    return toBooleans(res.valid);
  }

  async close() {
    if (this.closed) return;
    this.closed = true;
    addon.close(this.ctx);
  }

  canAcceptWork() {
    return true;
  }
}

module.exports = {
  addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, QueueError, sourceHash, checkBuildId, chunkifyMaximizeChunkSize, encodeJobs, checkSets, shardJobs, jobWork,
  encodeJobsBits, hasCommitteeSets, encodeSameMessage, mergeSameMessage, checkSameMessage, encodeSameMessageAgg, checkAggregateSameMessage,
  encodeSameMessageBits, hasCommitteeKeys, encodeAggregateSide, G2_IDENTITY_96,
  MAX_BUFFERED_SIGS, MAX_BUFFER_WAIT_MS, MAX_JOBS_CAN_ACCEPT_WORK, SHARD_MIN_SETS, PRIORITY_CUS, RESERVED_CAP, CONTEXTS_PER_DEVICE,
};
