"use strict";
// The Node side of tools/gen_napi_binding_golden.py: replays a seeded corpus through
// lodestar_amd/napi/index.js (over a stand-in `addon` object, no library) and through a
// copy of bgv.node linked against tools/bgv_record_stub.c, and prints the record as JSON.
//
//   node tools/napi_binding_golden.js <bgv.node built over the stub> <log file of the stub>
const assert = require("assert");
const crypto = require("crypto");
const fs = require("fs");
const path = require("path");

const NAPI = path.join(__dirname, "..", "lodestar_amd", "napi");
const [STUB_ADDON, LOG] = process.argv.slice(2);

// digests are the first 64 bits of the SHA-256, which keeps the file small
const sha = (x) => crypto.createHash("sha256").update(x).digest("hex").slice(0, 16);
const isTyped = (v) => ArrayBuffer.isView(v) && !(v instanceof DataView);
const typedRec = (v) => ({t: v.constructor.name, n: v.length, h: sha(Buffer.from(v.buffer, v.byteOffset, v.byteLength))});

// a value as the file holds it: typed arrays by constructor, length and digest, objects with their keys in order
function describe(v) {
  if (v === undefined) return "undefined";
  if (v === null || typeof v === "number" || typeof v === "boolean" || typeof v === "string") return v;
  if (isTyped(v)) return typedRec(v);
  if (Array.isArray(v)) return v.map(describe);
  if (v instanceof Error) return errRec(v);
  if (typeof v === "object" && Object.getPrototypeOf(v) === null) return "external";
  if (typeof v === "object") {
    const keys = Object.keys(v);
    if (keys.length === 0 && Object.getPrototypeOf(v) !== Object.prototype) return "external";
    const o = {};
    for (const k of keys) if (k !== "workerStartMs" && k !== "workerEndMs") o[k] = describe(v[k]);
    if ("workerStartMs" in v) o.endGeStart = v.workerEndMs >= v.workerStartMs;
    return {keys, v: o};
  }
  return typeof v;
}
const digestOf = (v) => sha(JSON.stringify(describe(v)));
const errRec = (e) => (e && e.constructor ? [e.constructor.name, e.message].concat(e.code ? [e.code] : []) : ["thrown", String(e)]);

function attempt(fn) {
  try {
    return {ok: describe(fn())};
  } catch (e) {
    return {throws: errRec(e)};
  }
}

async function attemptAsync(fn) {
  let p;
  try {
    p = fn();
  } catch (e) {
    return {throws: errRec(e)};
  }
  if (!p || typeof p.then !== "function") return {ok: describe(p)};
  try {
    return {resolves: describe(await p)};
  } catch (e) {
    return {rejects: errRec(e)};
  }
}

// ------------------------------------------------------------------ corpus
function rng(seed) {
  let s = seed >>> 0;
  return () => {
    s = (s + 0x6d2b79f5) >>> 0;
    let t = s;
    t = Math.imul(t ^ (t >>> 15), t | 1);
    t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
    return ((t ^ (t >>> 14)) >>> 0);
  };
}
const R = rng(0x5eed0b1e);
const bytes = (n) => Uint8Array.from({length: n}, () => R() & 0xff);
const key = () => (R() % 3 === 0 ? {raw: bytes(96)} : {index: R() % 100000});
const SIG_LENS = [96, 192, 96, 95, 96, 0, 192, 97];
const sig = (i) => bytes(SIG_LENS[i % SIG_LENS.length]);
const single = (i) => ({type: "single", pubkey: key(), signingRoot: bytes(32), signature: sig(i)});
const aggregate = (i, k) => ({type: "aggregate", pubkeys: Array.from({length: k}, key), signingRoot: bytes(32), signature: sig(i)});
function committee(i, len, list = i % 8) {
  const bits = bytes((len + 7) >> 3);
  bits[0] |= 1;
  return {type: "committee", committee: {list, offset: R() % 5000, length: len}, bits, signingRoot: bytes(32), signature: sig(i)};
}
const smSet = (i) => ({publicKey: key(), signature: sig(i)});
const smaSet = (i, k) => ({publicKeys: Array.from({length: k}, (_, q) => (q % 3 === 2 ? R() % 100000 : key())), signature: sig(i)});
const smbSet = (i, len) => { const c = committee(i, len); return {committee: c.committee, bits: c.bits, signature: c.signature}; };

const JOBS = {
  empty: [],
  emptyJob: [[]],
  oneSet: [[single(0)]],
  singles: [[single(0), single(1), single(2)], [single(3)]],
  mixed: [[single(4), aggregate(5, 4)], [], [aggregate(6, 1), aggregate(7, 7), single(8)]],
  rawOnly: [[{type: "single", pubkey: {raw: bytes(96)}, signingRoot: bytes(32), signature: sig(0)}]],
};
const JOBS_BITS = {
  ...JOBS,
  committees: [[committee(0, 128), committee(1, 77)], [committee(2, 1)]],
  everything: [[single(1), committee(3, 40), aggregate(2, 3)], [], [committee(4, 9)]],
};
const MSG = [bytes(32), bytes(32), bytes(32)];
const SM_GROUPS = {
  empty: [],
  oneSet: [{message: MSG[0], sets: [smSet(0)]}],
  groups: [{message: MSG[0], sets: [smSet(0), smSet(1), smSet(2)]}, {message: MSG[1], sets: [smSet(3), smSet(4)]}],
  emptyGroup: [{message: MSG[0], sets: []}],
};
const SMA_GROUPS = {
  empty: [],
  oneSet: [{message: MSG[0], sets: [smaSet(0, 1)]}],
  groups: [{message: MSG[0], sets: [smaSet(0, 4), smaSet(1, 3)]}, {message: MSG[2], sets: [smaSet(2, 6), smaSet(3, 1), smaSet(4, 2)]}],
  emptyGroup: [{message: MSG[0], sets: []}],
  emptyKeys: [{message: MSG[0], sets: [{publicKeys: [], signature: sig(0)}]}],
};
const SMB_GROUPS = {
  ...SMA_GROUPS,
  committees: [{message: MSG[0], sets: [smbSet(0, 128), smbSet(1, 33)]}, {message: MSG[1], sets: [smbSet(2, 8)]}],
  everything: [{message: MSG[1], sets: [smaSet(0, 3), smbSet(1, 20)]}, {message: MSG[2], sets: [smbSet(2, 5), smaSet(3, 2)]}],
  badBits: [{message: MSG[0], sets: [{committee: {list: 0, offset: 0, length: 20}, bits: bytes(2), signature: sig(0)}]}],
};

// ------------------------------------------------------- the JS layer's addon
// what index.js loads instead of bgv.node: every method notes its name and the digest of what it got
// and answers from the batch's own sizes, with fixed worker times
const calls = [];
const WORKER = {deviceMs: 1.25, workerStartMs: 100, workerEndMs: 104};
function fakeVerify(name, extra = {}) {
  return (ctx, b) => {
    calls.push([name, ctx, digestOf(b)]);
    const n = b.jobOffsets.length - 1;
    return {results: Int32Array.from({length: n}, (_, i) => (i % 5 === 4 ? -3 : i % 3 === 2 ? 0 : 1)), batchRetries: 1, batchSigsSuccess: n,
      pubkeysAggregated: 9, ...WORKER, hashes: n + 1, millerPairs: n + 2, ...extra};
  };
}
function fakeSm(name, kind) {
  return (ctx, b) => {
    calls.push([name, ctx, digestOf(b)]);
    const g = b.groupOffsets.length - 1;
    const n = b.groupOffsets[g];
    const r = {valid: Uint8Array.from({length: n}, (_, i) => (i % 3 === 1 ? 0 : 1)), codes: new Int32Array(n), segments: g, hashes: g, pairs: n,
      groupsRetried: n > 2 ? 1 : 0, setsRetried: 0};
    if (kind === "bits") r.pubkeysAggregated = 1000 + n;
    if (kind === "aggregate") {
      r.aggSigs = Uint8Array.from({length: 96 * g}, (_, i) => i & 0xff);
      r.aggCount = Uint32Array.from({length: g}, (_, i) => i + 1);
      r.aggCode = Int32Array.from({length: g}, (_, i) => (i % 3 === 2 ? 1 : 0));
    }
    return {...r, ...WORKER};
  };
}
const note = (name, ret) => (...a) => { calls.push([name, ...a.map((x) => (isTyped(x) ? digestOf(x) : x))]); return typeof ret === "function" ? ret(...a) : ret; };
const later = (f) => (...a) => { const r = f(...a); return new Promise((res) => setImmediate(() => res(r))); };
let nextCtx = 0;
const fake = {
  buildId: () => ID,
  open: (d, cu) => { calls.push(["open", d, cu]); return `ctx${nextCtx++}`; },
  close: note("close"), pubkeysSet: note("pubkeysSet"), setIndexList: note("setIndexList"), setIndexListSums: note("setIndexListSums"),
  pairMerge: note("pairMerge"), smRetry: note("smRetry"), codeName: (c) => `BLST_CODE_${c}`,
  smRetryStats: note("smRetryStats", {mode: 1, segments: 2, subs: 3, subsFailed: 1, leaves: 4, pairs: 5, hashes: 6}),
  verify: later(fakeVerify("verify")), verifySync: fakeVerify("verifySync"),
  verifyBits: later(fakeVerify("verifyBits")), verifyBitsSync: fakeVerify("verifyBitsSync"),
  partial: later(fakeVerify("partial", {miller: new Uint8Array(576).fill(5), ok: true})),
  partialFinish: later((ctx) => { calls.push(["partialFinish", ctx]); return {results: new Int32Array(64).fill(1), batchRetries: 0, batchSigsSuccess: 0, pubkeysAggregated: 0, ...WORKER}; }),
  combineFinal: later((ctx, m) => { calls.push(["combineFinal", ctx, digestOf(m)]); return false; }),
  verifySameMessage: later(fakeSm("verifySameMessage")), verifySameMessageSync: fakeSm("verifySameMessageSync"),
  verifySameMessageAggregate: later(fakeSm("verifySameMessageAggregate", "aggregate")),
  verifySameMessageAggregateSync: fakeSm("verifySameMessageAggregateSync", "aggregate"),
  verifySameMessageAgg: later(fakeSm("verifySameMessageAgg")), verifySameMessageAggSync: fakeSm("verifySameMessageAggSync"),
  verifySameMessageBits: later(fakeSm("verifySameMessageBits", "bits")), verifySameMessageBitsSync: fakeSm("verifySameMessageBitsSync", "bits"),
};
// index.js checks the library's build id while it loads, before its sourceHash is exported
const ID = (() => {
  const root = path.join(__dirname, "..");
  const csrc = path.join(root, "lodestar_amd", "csrc");
  const files = fs.readdirSync(csrc).filter((f) => f.endsWith(".h") || f.endsWith(".hip")).sort().map((f) => "lodestar_amd/csrc/" + f).concat(["include/bgv.h"]);
  const h = crypto.createHash("sha256");
  for (const rel of files) {
    const data = fs.readFileSync(path.join(root, rel));
    const len = Buffer.alloc(8);
    len.writeUInt32LE(data.length % 0x100000000, 0);
    len.writeUInt32LE(Math.floor(data.length / 0x100000000), 4);
    h.update(Buffer.concat([Buffer.from(rel + "\0"), len, data]));
  }
  return h.digest("hex");
})();
// index.js gets the stand-in where it asks for its bgv.node, which need not have been built
const Module = require("module");
const load = Module._load;
Module._load = function (request, ...rest) {
  return path.resolve(request) === path.join(NAPI, "bgv.node") ? fake : load.call(this, request, ...rest);
};
if (!process.env.UV_THREADPOOL_SIZE) process.env.UV_THREADPOOL_SIZE = "16"; // index.js warns about a small pool
const I = require(path.join(NAPI, "index.js"));
assert.strictEqual(I.sourceHash(), ID);
assert.strictEqual(I.addon, fake);

// --------------------------------------------------------------- JS layer
// sums of seconds are rounded: the order in which device calls of one run settle may change their last bits
const round = (x) => Number(x.toPrecision(9));
// a metrics object: the digest of its keys in order (pool/construct holds the list itself) and every entry that is not zero
function metricsRec(m, full = false) {
  const o = {};
  for (const k of Object.keys(m)) {
    // the two histograms fed from the wall clock keep their count only
    if (k === "lodestar_bls_thread_pool_queue_job_wait_time_seconds" || k === "lodestar_bls_thread_pool_main_thread_time_seconds") o[k] = {count: m[k].count};
    else if (typeof m[k] === "number") o[k] = round(m[k]);
    else o[k] = {count: m[k].count, sum: round(m[k].sum)};
    if (o[k] === 0 || (o[k] && o[k].count === 0)) delete o[k];
  }
  return {keys: full ? Object.keys(m) : sha(Object.keys(m).join()), v: o};
}
const takeCalls = () => calls.splice(0, calls.length);

function encoders() {
  const out = {};
  const each = (name, fn, corpus) => { for (const c of Object.keys(corpus)) out[`${name}/${c}`] = attempt(() => fn(corpus[c])); };
  each("encodeJobs", I.encodeJobs, JOBS);
  each("encodeJobs", I.encodeJobs, {committeeRefused: JOBS_BITS.committees, numericKey: [[{type: "aggregate", pubkeys: [7, 8], signingRoot: bytes(32), signature: sig(0)}]]});
  each("encodeJobsBits", I.encodeJobsBits, JOBS_BITS);
  each("encodeJobsBits", I.encodeJobsBits, {numericKey: [[{type: "aggregate", pubkeys: [7, 8], signingRoot: bytes(32), signature: sig(0)}]],
    badBits: [[{type: "committee", committee: {list: 0, offset: 0, length: 20}, bits: bytes(2), signingRoot: bytes(32), signature: sig(0)}]]});
  each("encodeSameMessage", I.encodeSameMessage, SM_GROUPS);
  each("encodeSameMessageAgg", I.encodeSameMessageAgg, SMA_GROUPS);
  each("encodeSameMessageBits", I.encodeSameMessageBits, SMB_GROUPS);
  const aggCalls = [
    {sets: SM_GROUPS.groups[0].sets, message: MSG[0]},
    {sets: SM_GROUPS.groups[1].sets, message: MSG[0], agg: {previous: bytes(96), take: [true, false]}},
    {sets: [smSet(5)], message: MSG[1], agg: {previous: null, take: null}},
    {sets: [smSet(6), smSet(7)], message: MSG[0]},
    {sets: [smSet(8), smSet(9)], message: MSG[2], agg: {previous: null, take: [0, 1]}},
  ];
  for (const [name, cs] of [["all", aggCalls], ["plainOnly", [aggCalls[0], aggCalls[3]]], ["oneAgg", [aggCalls[1]]], ["none", []]]) {
    const merged = I.mergeSameMessage(cs);
    const n = cs.reduce((a, c) => a + c.sets.length, 0);
    out[`encodeAggregateSide/${name}`] = attempt(() => I.encodeAggregateSide(cs, merged, n));
    out[`mergeSameMessage/${name}`] = {where: merged.where, groupOf: merged.groupOf, sizes: merged.groups.map((g) => g.sets.length),
      messages: merged.groups.map((g) => sha(g.message))};
  }
  return out;
}

function refusals() {
  const out = {};
  const t = (name, fn) => { out[name] = attempt(fn); };
  const c = (over = {}, o = {}) => ({type: "committee", committee: {list: 1, offset: 3, length: 16, ...over}, bits: Uint8Array.of(1, 0), signingRoot: bytes(32), signature: sig(0), ...o});
  const setCases = {
    ok: [single(0), aggregate(1, 2), c()], emptyAggregate: [{type: "aggregate", pubkeys: [], signingRoot: bytes(32), signature: sig(0)}],
    noPubkey: [{type: "single", signingRoot: bytes(32), signature: sig(0)}], nullKey: [{type: "aggregate", pubkeys: [key(), null], signingRoot: bytes(32), signature: sig(0)}],
    rawLength: [{type: "single", pubkey: {raw: bytes(48)}, signingRoot: bytes(32), signature: sig(0)}], shortRoot: [{...single(0), signingRoot: bytes(31)}],
    noRoot: [{...single(0), signingRoot: null}], committeeNoBits: [c({}, {bits: null})], committeeNoCommittee: [c({}, {committee: null})],
    committeeList: [c({list: 8})], committeeListNegative: [c({list: -1})], committeeOffset: [c({offset: -1})], committeeLength: [c({length: -1})],
    committeeOverflow: [c({offset: 0xffffffff})], committeeBitsLength: [c({length: 17})], committeeNoBitSet: [c({}, {bits: Uint8Array.of(0, 0)})],
    committeeShortRoot: [c({}, {signingRoot: bytes(5)})], numericKey: [{type: "aggregate", pubkeys: [5], signingRoot: bytes(32), signature: sig(0)}],
  };
  for (const k of Object.keys(setCases)) t(`checkSets/${k}`, () => I.checkSets(setCases[k]));
  const sm = {ok: [smSet(0)], noKey: [{signature: sig(0)}], nullSet: [null], rawLength: [{publicKey: {raw: bytes(95)}, signature: sig(0)}], empty: []};
  for (const k of Object.keys(sm)) t(`checkSameMessage/${k}`, () => I.checkSameMessage(sm[k], MSG[0]));
  t("checkSameMessage/shortMessage", () => I.checkSameMessage(sm.ok, bytes(31)));
  t("checkSameMessage/noMessage", () => I.checkSameMessage(sm.ok, null));
  const cs = (over = {}, o = {}) => ({committee: {list: 1, offset: 3, length: 16, ...over}, bits: Uint8Array.of(1, 0), signature: sig(0), ...o});
  const sma = {
    ok: [smaSet(0, 3), cs()], numericKey: [{publicKeys: [5, 6], signature: sig(0)}], noKeys: [{signature: sig(0)}], emptyKeys: [{publicKeys: [], signature: sig(0)}],
    nullSet: [null], nullKey: [{publicKeys: [key(), null], signature: sig(0)}], undefinedKey: [{publicKeys: [undefined], signature: sig(0)}],
    rawLength: [{publicKeys: [{raw: bytes(97)}], signature: sig(0)}], committeeNoBits: [cs({}, {bits: null})], committeeList: [cs({list: 8})],
    committeeOffset: [cs({offset: -1})], committeeLength: [cs({length: -1})], committeeOverflow: [cs({offset: 0xffffffff})],
    committeeBitsLength: [cs({length: 17})], committeeNoBitSet: [cs({}, {bits: Uint8Array.of(0, 0)})],
  };
  for (const k of Object.keys(sma)) t(`checkAggregateSameMessage/${k}`, () => I.checkAggregateSameMessage(sma[k], MSG[0]));
  t("checkAggregateSameMessage/shortMessage", () => I.checkAggregateSameMessage(sma.ok, bytes(33)));
  for (const k of Object.keys(JOBS_BITS)) out[`hasCommitteeSets/${k}`] = I.hasCommitteeSets(JOBS_BITS[k]);
  for (const k of Object.keys(SMB_GROUPS)) out[`hasCommitteeKeys/${k}`] = I.hasCommitteeKeys(SMB_GROUPS[k]);
  return out;
}

async function verifiers() {
  const out = {};
  const settle = (ps) => Promise.all(ps.map((p) => attemptAsync(() => p)));
  const run = async (name, make, body) => {
    nextCtx = 0;
    takeCalls();
    const v = make();
    const results = await body(v);
    out[name] = {results, calls: takeCalls(), metrics: metricsRec(v.metricsSnapshot ? v.metricsSnapshot() : v.metrics, /construct|single\/close/.test(name))};
    if ("smDeviceCalls" in v) out[name].deviceCalls = [v.smDeviceCalls, v.smaDeviceCalls];
    await v.close();
  };
  const pool = (o = {}) => () => new I.BlsGpuVerifier({device: 0, contextsPerDevice: 2, ...o});
  const one = (o = {}) => () => new I.BlsGpuSingleThreadVerifier(o);
  const many = (n, f) => Array.from({length: n}, (_, i) => f(i));

  await run("pool/construct", pool({pairMerge: true, smRetry: true, devices: [0, 1]}), async () => []);
  await run("pool/verifySignatureSets", pool(), (v) => settle([
    v.verifySignatureSets([single(0), aggregate(1, 3)]), v.verifySignatureSets([single(2), committee(3, 24)]),
    v.verifySignatureSets([single(4)], {verifyOnMainThread: true}), v.verifySignatureSets([committee(5, 9)], {verifyOnMainThread: true}),
    v.verifySignatureSets([]), v.verifySignatureSets([{type: "aggregate", pubkeys: [], signingRoot: bytes(32), signature: sig(0)}]),
    v.verifySignatureSets(many(300, single)),
  ]));
  await run("pool/verifySignatureSets/batchable", pool(), (v) => settle(many(6, (i) => v.verifySignatureSets(many(7, single), {batchable: true}))));
  await run("pool/verifySignatureSets/sharded", pool({devices: [0, 1], shardMinSets: 8}), (v) => settle(many(4, (i) => v.verifySignatureSets(many(5, single)))));
  await run("pool/verifySignatureSetsSync", pool(), async (v) => [attempt(() => v.verifySignatureSetsSync([single(0)])), attempt(() => v.verifySignatureSetsSync([committee(1, 8)]))]);
  await run("pool/allMultiThread", pool({blsVerifyAllMultiThread: true}), async (v) => [
    await attemptAsync(() => v.verifySignatureSets([single(0)], {verifyOnMainThread: true})), attempt(() => v.verifySignatureSetsSync([single(0)]))]);
  // a buffered burst that crosses MAX_BUFFERED_SIGS, then two calls left to the buffer's timer
  await run("pool/sameMessage/burst", pool(), (v) => settle(many(6, (i) => v.verifySignatureSetsSameMessage(many(7, smSet), MSG[i % 2], {batchable: true}))));
  await run("pool/sameMessage/nonBatchable", pool(), (v) => settle([v.verifySignatureSetsSameMessage(many(3, smSet), MSG[0]), v.verifySignatureSetsSameMessage([], MSG[0]),
    v.verifySignatureSetsSameMessage([smSet(0)], bytes(3))]));
  await run("pool/sameMessage/oneAggregateAmongPlain", pool(), (v) => settle([
    v.verifySignatureSetsSameMessage(many(3, smSet), MSG[0]), v.verifyAndAggregateSameMessage(many(4, smSet), MSG[0], {previous: bytes(96), take: [true, false, true, true]}),
    v.verifySignatureSetsSameMessage(many(2, smSet), MSG[0]), v.verifyAndAggregateSameMessage([smSet(0)], MSG[1]),
    v.verifyAndAggregateSameMessage([smSet(1)], MSG[1]), v.verifyAndAggregateSameMessage([], MSG[1], {previous: bytes(96)}),
    v.verifyAndAggregateSameMessage([], MSG[1]), v.verifyAndAggregateSameMessage([smSet(1)], MSG[1], {take: []}),
  ]));
  await run("pool/sameMessage/aggregateBurst", pool(), (v) => settle(many(5, (i) => v.verifyAndAggregateSameMessage(many(9, smSet), MSG[i % 2], {batchable: true}))));
  await run("pool/aggSameMessage/burst", pool(), (v) => settle(many(6, (i) => v.verifyAggregateSetsSameMessage(many(7, (q) => smaSet(q, 1 + (q % 4))), MSG[i % 3], {batchable: true}))));
  await run("pool/aggSameMessage/nonBatchable", pool(), (v) => settle([v.verifyAggregateSetsSameMessage([smaSet(0, 4), smaSet(1, 2)], MSG[0]),
    v.verifyAggregateSetsSameMessage([], MSG[0]), v.verifyAggregateSetsSameMessage([{publicKeys: []}], MSG[0])]));
  await run("pool/aggSameMessage/mergedWithCommittee", pool(), (v) => settle([v.verifyAggregateSetsSameMessage([smaSet(0, 4), smaSet(1, 2)], MSG[0]),
    v.verifyAggregateSetsSameMessage([smbSet(2, 64), smaSet(3, 3)], MSG[1]), v.verifyAggregateSetsSameMessage([smaSet(4, 1)], MSG[0])]));
  await run("pool/sameMessage/smallDeviceBatch", pool({maxSetsPerDeviceBatch: 8}), (v) => settle([
    v.verifySignatureSetsSameMessage(many(5, smSet), MSG[0]), v.verifySignatureSetsSameMessage(many(5, smSet), MSG[1])]));
  await run("pool/aggSameMessage/smallDeviceBatch", pool({maxSetsPerDeviceBatch: 8}), (v) => settle([
    v.verifyAggregateSetsSameMessage(many(6, (q) => smaSet(q, 2)), MSG[0]), v.verifyAggregateSetsSameMessage(many(6, (q) => smaSet(q, 2)), MSG[1])]));
  await run("pool/canAcceptWork", pool({maxSetsPerDeviceBatch: 20}), async (v) => {
    const seen = [v.canAcceptWork()];
    const ps = [v.verifySignatureSetsSameMessage(many(11, smSet), MSG[0], {batchable: true})];
    seen.push(v.canAcceptWork());
    ps.push(v.verifyAggregateSetsSameMessage(many(11, (q) => smaSet(q, 2)), MSG[0], {batchable: true}));
    seen.push(v.canAcceptWork());
    ps.push(v.verifySignatureSets(many(8, single), {batchable: true}));
    seen.push(v.canAcceptWork());
    // one buffer after the other, so that the device calls of the three queues do not interleave
    const flush = [v.flushSameMessage, v.flushSameMessageAgg, v.runBufferedJobs];
    const results = [];
    for (let k = 0; k < 3; k++) {
      flush[k]();
      seen.push(v.canAcceptWork());
      results.push(await attemptAsync(() => ps[k]));
    }
    return [seen, results];
  });
  await run("pool/close", pool(), async (v) => {
    const ps = [v.verifySignatureSetsSameMessage(many(3, smSet), MSG[0], {batchable: true}), v.verifySignatureSetsSameMessage(many(3, smSet), MSG[0]),
      v.verifyAggregateSetsSameMessage([smaSet(0, 2)], MSG[0], {batchable: true}), v.verifyAggregateSetsSameMessage([smaSet(0, 2)], MSG[0]),
      v.verifySignatureSets([single(0)], {batchable: true}), v.verifySignatureSets([single(0)])];
    const queued = settle(ps);
    await v.close();
    return settle([v.verifySignatureSets([single(0)]), v.verifySignatureSetsSameMessage([smSet(0)], MSG[0]), v.verifyAndAggregateSameMessage([smSet(0)], MSG[0]),
      v.verifyAggregateSetsSameMessage([smaSet(0, 1)], MSG[0])]).then(async (r) => (await queued).concat(r, [attempt(() => v.verifySignatureSetsSync([single(0)])), v.canAcceptWork()]));
  });
  await run("single/all", one({pairMerge: true, smRetry: true}), async (v) => {
    v.syncPubkeys(3, bytes(96));
    v.pubkeysSet(0, bytes(96), 1);
    v.setIndexList(2, Uint32Array.of(1, 2, 3), {sums: true});
    v.setIndexList(3, new Uint32Array(0), {sums: true});
    return settle([v.verifySignatureSets([single(0), aggregate(1, 3)]), v.verifySignatureSets([committee(2, 12), single(3)]),
      v.verifySignatureSets([{type: "aggregate", pubkeys: [], signingRoot: bytes(32), signature: sig(0)}]), v.verifySignatureSets([]),
      v.verifySignatureSetsSameMessage(many(4, smSet), MSG[0]), v.verifySignatureSetsSameMessage([], MSG[0]),
      v.verifyAndAggregateSameMessage(many(4, smSet), MSG[0], {previous: bytes(96), take: [1, 0, 1, 1]}), v.verifyAndAggregateSameMessage(many(2, smSet), MSG[0]),
      v.verifyAndAggregateSameMessage([], MSG[0]), v.verifyAndAggregateSameMessage([], MSG[0], {previous: bytes(96)}),
      v.verifyAndAggregateSameMessage([smSet(0)], MSG[0], {previous: bytes(9)}),
      v.verifyAggregateSetsSameMessage([smaSet(0, 3), smaSet(1, 2)], MSG[1]), v.verifyAggregateSetsSameMessage([smaSet(0, 3), smbSet(1, 30)], MSG[1]),
      v.verifyAggregateSetsSameMessage([], MSG[1]), v.verifyAggregateSetsSameMessage([null], MSG[1])]).then((r) => r.concat([v.canAcceptWork()]));
  });
  // checkAggregateOpts is not exported: every option alone through verifyAndAggregateSameMessage of both classes
  const aggregateOpts = async (v) => {
    const opts = {none: {}, ok: {previous: bytes(96), take: [true, false]}, shortPrevious: {previous: bytes(95)}, longPrevious: {previous: bytes(97)},
      takeShort: {take: [true]}, takeLong: {take: [true, false, true]}, nulls: {previous: null, take: null}, undefineds: {previous: undefined, take: undefined}};
    const r = {};
    for (const k of Object.keys(opts)) {
      r[k] = await attemptAsync(() => v.verifyAndAggregateSameMessage([smSet(0), smSet(1)], MSG[0], opts[k]));
      r[k + "/noSets"] = await attemptAsync(() => v.verifyAndAggregateSameMessage([], MSG[0], opts[k]));
    }
    return r;
  };
  await run("checkAggregateOpts/pool", pool(), aggregateOpts);
  await run("checkAggregateOpts/single", one(), aggregateOpts);
  await run("single/close", one(), async (v) => {
    await v.close();
    return settle([v.verifySignatureSets([single(0)]), v.verifySignatureSetsSameMessage([smSet(0)], MSG[0]), v.verifyAndAggregateSameMessage([smSet(0)], MSG[0]),
      v.verifyAggregateSetsSameMessage([smaSet(0, 1)], MSG[0])]);
  });
  return out;
}

// ------------------------------------------------------------ addon layer
const A = STUB_ADDON ? require(path.resolve(STUB_ADDON)) : null;
function takeLog() {
  const lines = fs.existsSync(LOG) ? fs.readFileSync(LOG, "utf8").split("\n").filter((l) => l) : [];
  fs.writeFileSync(LOG, "");
  return lines.map((l) => l.replace(/\b([0-9a-f]{16})[0-9a-f]{48}\b/g, "$1"));
}
// one call: its outcome and what the library saw; `fail` scripts an error of that library entry
async function call(fn, fail = null) {
  if (fail) process.env.BGV_RECORD_FAIL = fail;
  const r = await attemptAsync(fn);
  delete process.env.BGV_RECORD_FAIL;
  // `lib` is left out where the library saw nothing
  const lib = takeLog();
  return lib.length ? {...r, lib} : r;
}
// a reader case in short: the refusal, or one digest over the value and what the library saw
const brief = (r) => (r.throws || r.rejects ? {throws: r.throws || r.rejects, lib: r.lib} : {ok: sha(JSON.stringify([r.resolves || r.ok, r.lib]))});

// the readers' batches, one per entry kind, from the encoders over the corpus
const KINDS = {
  verify: {lib: "bgv_verify", batch: () => I.encodeJobs(JOBS.mixed), empty: () => I.encodeJobs([])},
  partial: {lib: "bgv_partial", noSync: true, batch: () => I.encodeJobs(JOBS.singles), empty: () => I.encodeJobs([])},
  verifyBits: {lib: "bgv_verify_bits", batch: () => I.encodeJobsBits(JOBS_BITS.everything), empty: () => I.encodeJobsBits([])},
  verifySameMessage: {lib: "bgv_verify_same_message", batch: () => I.encodeSameMessage(SM_GROUPS.groups), empty: () => I.encodeSameMessage([])},
  verifySameMessageAggregate: {lib: "bgv_verify_same_message_aggregate", empty: () => ({...I.encodeSameMessage([]), take: new Uint8Array(1), prevSigs: new Uint8Array(96)}),
    batch: () => ({...I.encodeSameMessage(SM_GROUPS.groups), take: Uint8Array.of(1, 0, 1, 1, 1), prevSigs: bytes(192)})},
  verifySameMessageAgg: {lib: "bgv_verify_same_message_agg", batch: () => I.encodeSameMessageAgg(SMA_GROUPS.groups), empty: () => I.encodeSameMessageAgg([])},
  verifySameMessageBits: {lib: "bgv_verify_same_message_bits", batch: () => I.encodeSameMessageBits(SMB_GROUPS.everything), empty: () => I.encodeSameMessageBits([])},
};
const OTHER_TYPE = (v) => (v instanceof Uint8Array ? new Uint32Array(v.length) : v instanceof Uint32Array ? new Int32Array(v.length) : new Uint8Array(v.length));
// every way a reader can refuse one field, each alone
function mutations(batch) {
  const out = [];
  const withField = (k, v) => { const b = {...batch}; b[k] = v; return b; };
  for (const k of Object.keys(batch)) {
    const without = {...batch};
    delete without[k];
    out.push([`${k}/missing`, without], [`${k}/null`, withField(k, null)], [`${k}/undefined`, withField(k, undefined)],
      [`${k}/wrongType`, withField(k, OTHER_TYPE(batch[k]))], [`${k}/plainArray`, withField(k, Array.from(batch[k]))], [`${k}/empty`, withField(k, batch[k].slice(0, 0))],
      [`${k}/shorterByOne`, withField(k, batch[k].slice(0, batch[k].length - 1))]);
    if (/Offsets$/.test(k)) {
      const up = batch[k].slice();
      up[up.length - 1] += 1;
      const far = batch[k].slice();
      far[far.length - 1] = 0xffffffff;
      out.push([`${k}/endsOneLater`, withField(k, up)], [`${k}/endsFar`, withField(k, far)], [`${k}/oneEntry`, withField(k, batch[k].slice(0, 1))]);
    }
    if (k === "src") {
      const longer = new Uint32Array(batch[k].length + 1);
      longer.set(batch[k]);
      out.push([`${k}/notAMultipleOfFour`, withField(k, longer)], [`${k}/oneSetMore`, withField(k, Uint32Array.from([...batch[k], 0xffffffff, 0, 0, 0]))]);
    }
  }
  return out;
}

// a first argument that is no context (none, an object, a number, null): one entry where all four are refused alike
const NOT_CTX = {none: [], object: [{}], number: [5], nul: [null]};
async function notContext(out, name, fn) {
  const r = {};
  for (const k of Object.keys(NOT_CTX)) r[k] = await call(() => fn(NOT_CTX[k]));
  const all = Object.keys(r).map((k) => JSON.stringify(r[k]));
  if (all.every((x) => x === all[0])) out[`${name}/notContext`] = r.none;
  else for (const k of Object.keys(r)) out[`${name}/notContext/${k}`] = r[k];
}

async function addonLayer() {
  const out = {};
  takeLog();
  out.exports = Object.keys(A);
  out["abiVersion"] = await call(() => A.abiVersion());
  out["buildId"] = await call(() => A.buildId());
  for (const c of [0, 3, 8, -1]) out[`codeName/${c}`] = await call(() => A.codeName(c));
  out["codeName/none"] = await call(() => A.codeName());
  const opens = {none: [], device: [2], cuSplit: [1, 32], bulk: [0, -32], cfg: [0, 0, {split: 1, miller: 2, hashDedup: 1, millerSteps: 0}], cfgNull: [0, 0, null],
    cfgUndefined: [0, 0, undefined], cfgOtherKey: [0, 0, {split: 1, lanes: 3}], cfgNotObject: [0, 0, 5], cfgNotNumber: [0, 0, {split: "x"}], deviceNotNumber: ["x"]};
  for (const k of Object.keys(opens)) out[`open/${k}`] = await call(() => A.open(...opens[k]));
  out["open/fails"] = await call(() => A.open(0), "bgv_open_cfg");

  const ctx = A.open(0);
  const closed = A.open(0);
  A.close(closed);
  takeLog();
  // every (ctx, ...) entry: a good call, a scripted failure of its library entry, a closed context and a non-context
  const plain = {
    pubkeysSet: {lib: "bgv_pubkeys_set", args: {compressed: [5, bytes(96), 0], uncompressed: [0, bytes(192), 1], odd: [0, bytes(100), 0], empty: [0, new Uint8Array(0), 0],
      notTyped: [0, [1, 2], 0], wrongType: [0, new Uint32Array(12), 0], noFormat: [0, bytes(48)], firstNotNumber: ["a", bytes(48), 0]}},
    pubkeysCount: {lib: "bgv_pubkeys_count", args: {ok: []}},
    pubkeysValidate: {lib: "bgv_pubkeys_validate", args: {ok: [bytes(48 * 5)], odd: [bytes(100)], empty: [new Uint8Array(0)], wrongType: [new Uint16Array(48)], none: []}},
    setIndexList: {lib: "bgv_index_list_set", args: {ok: [2, Uint32Array.of(5, 6, 7)], empty: [2, new Uint32Array(0)], wrongType: [2, new Uint8Array(4)], noList: [2], idNotNumber: ["a", new Uint32Array(1)]}},
    indexListLen: {lib: "bgv_index_list_len", args: {ok: [3], none: []}},
    setIndexListSums: {lib: "bgv_index_list_sums", args: {on: [1, true], off: [1, false], number: [1, 1], none: [1]}},
    indexListHasSums: {lib: "bgv_index_list_has_sums", args: {odd: [3], even: [4], none: []}},
    hashStats: {lib: "bgv_hash_stats", args: {ok: []}}, pairStats: {lib: "bgv_pair_stats", args: {ok: []}},
    smRetryStats: {lib: "bgv_sm_retry_stats", args: {ok: []}}, bitsPathStats: {lib: "bgv_bits_path_stats", args: {ok: []}},
    pairMerge: {lib: "bgv_pair_merge", args: {true: [true], false: [false], one: [1], two: [2], zero: [0], none: [], string: ["1"], nul: [null]}},
    smRetry: {lib: "bgv_sm_retry", args: {true: [true], false: [false], one: [1], two: [2], zero: [0], none: [], string: ["1"], nul: [null]}},
    combineFinal: {lib: "bgv_combine_final", args: {two: [bytes(1152)], one: [bytes(576)], empty: [new Uint8Array(0)], notAMultiple: [bytes(575)], wrongType: [new Uint32Array(576)], none: [], nul: [null]}},
    partialFinish: {lib: "bgv_partial_finish", args: {nothingPending: []}},
  };
  for (const name of Object.keys(plain)) {
    const p = plain[name];
    for (const k of Object.keys(p.args)) out[`${name}/${k}`] = await call(() => A[name](ctx, ...p.args[k]));
    const first = p.args[Object.keys(p.args)[0]];
    out[`${name}/fails`] = await call(() => A[name](ctx, ...first), p.lib);
    out[`${name}/closed`] = await call(() => A[name](closed, ...first));
    await notContext(out, name, (bad) => A[name](...bad, ...first));
  }
  out["close/notContext"] = await call(() => A.close({}));
  out["close/closed"] = await call(() => A.close(closed));

  for (const name of Object.keys(KINDS)) {
    const kind = KINDS[name];
    for (const fn of kind.noSync ? [name] : [name, name + "Sync"]) {
      const batch = kind.batch();
      out[`${fn}/batch`] = await call(() => A[fn](ctx, batch));
      out[`${fn}/empty`] = await call(() => A[fn](ctx, kind.empty()));
      out[`${fn}/fails`] = await call(() => A[fn](ctx, batch), kind.lib);
      out[`${fn}/closed`] = await call(() => A[fn](closed, batch));
      await notContext(out, fn, (bad) => A[fn](...bad, batch));
      out[`${fn}/noBatch`] = await call(() => A[fn](ctx));
      out[`${fn}/batchNotObject`] = await call(() => A[fn](ctx, 5));
      // a Sync case that equals the async one (a throw for a rejection, a value for a resolution) is only counted
      let equal = 0;
      for (const [k, b] of mutations(batch)) {
        const r = brief(await call(() => A[fn](ctx, b)));
        if (fn !== name && JSON.stringify(r) === JSON.stringify(out[`${name}/${k}`])) equal++;
        else out[`${fn}/${k}`] = r;
      }
      if (fn !== name) out[`${fn}/casesEqualToAsync`] = equal;
      // the counters read under the call's lock fail the call
      if (/^(verify|verifyBits|partial)(Sync)?$/.test(fn)) {
        out[`${fn}/hashStatsFail`] = await call(() => A[fn](ctx, batch), "bgv_hash_stats");
        out[`${fn}/pairStatsFail`] = await call(() => A[fn](ctx, batch), "bgv_pair_stats");
      }
      if (/Bits/.test(fn) && /SameMessage/.test(fn)) out[`${fn}/pathStatsFail`] = await call(() => A[fn](ctx, batch), "bgv_bits_path_stats");
    }
  }
  out["partial/lastStatsFail"] = await call(() => A.partial(ctx, KINDS.partial.batch()), "bgv_last_stats");
  // partial, then partialFinish sized from it; a batch whose async call is in flight while its arrays are overwritten
  out["partialThenFinish"] = [await call(() => A.partial(ctx, KINDS.partial.batch())), await call(() => A.partialFinish(ctx)), await call(() => A.partialFinish(ctx), "bgv_partial_finish")];
  const b = KINDS.verify.batch();
  const pending = A.verify(ctx, b);
  b.jobOffsets.fill(0xffffffff);
  b.pkOffsets.fill(0xffffffff);
  out["verify/offsetsOverwrittenInFlight"] = await call(() => pending);
  out["close"] = await call(() => A.close(ctx));
  out["close/twice"] = await call(() => A.close(ctx));
  return out;
}

(async () => {
  const rec = {generator: "tools/gen_napi_binding_golden.py", encoders: encoders(), refusals: refusals(), verifiers: await verifiers(),
    exports: {index: Object.keys(I)}};
  if (A) rec.addon = await addonLayer();
  process.stdout.write(JSON.stringify(rec));
})().catch((e) => { console.error(e); process.exit(1); });
