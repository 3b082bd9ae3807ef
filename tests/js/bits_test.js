"use strict";
// Committee signature sets ({type: "committee", committee: {list, offset, length}, bits}) through the N-API addon.
//   node bits_test.js --host   the encoder against intersectValues, the routing rule and the caller-side checks, no device
//   node bits_test.js DIR      those, then on the GPU: both Node classes on a 40-set mixed batch against the
//                              explicit-index call on the same sets
// The signed jobs come from tests/test_napi_bits.py (DIR: table96.bin and jobs.json).  Exits non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeJobs, encodeJobsBits, hasCommitteeSets, checkSets} =
  require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

// BitArray.intersectValues: the values whose bit is set
function intersectValues(bits, length, values) {
  assert.strictEqual(values.length, length);
  assert.strictEqual(bits.length, (length + 7) >> 3);
  const out = [];
  for (let j = 0; j < length; j++) if ((bits[j >> 3] >> (j & 7)) & 1) out.push(values[j]);
  return out;
}

// the same set with its keys spelled out: what a caller builds today
function explicitSet(s, lists) {
  if (s.type !== "committee") return s;
  const c = s.committee;
  const rows = intersectValues(s.bits, c.length, Array.from(lists[c.list].subarray(c.offset, c.offset + c.length)));
  return {type: "aggregate", pubkeys: rows.map((index) => ({index})), signingRoot: s.signingRoot, signature: s.signature};
}

function hostChecks() {
  const root = (k) => new Uint8Array(32).fill(k);
  const sig = (b, n = 96) => new Uint8Array(n).fill(b);
  const raw = Uint8Array.from({length: 96}, (_, k) => k);
  const lists = {0: Uint32Array.from({length: 300}, (_, k) => (k * 7919) % 4400), 2: Uint32Array.from({length: 64}, (_, k) => 4399 - k)};
  const bits13 = Uint8Array.from([0b10100101, 0b00010010]);
  const bits64 = Uint8Array.from({length: 8}, (_, k) => (k * 37 + 1) & 0xff);
  const jobs = [
    [{type: "single", pubkey: {index: 11}, signingRoot: root(1), signature: sig(0xa1)},
      {type: "committee", committee: {list: 0, offset: 17, length: 13}, bits: bits13, signingRoot: root(2), signature: sig(0xa2)},
      {type: "aggregate", pubkeys: [{index: 5}, {raw}, {index: 3}], signingRoot: root(3), signature: sig(0xa3, 192)}],
    [{type: "committee", committee: {list: 2, offset: 0, length: 64}, bits: bits64, signingRoot: root(4), signature: sig(0xa4, 7)}],
  ];
  assert.strictEqual(hasCommitteeSets(jobs), true);
  const e = encodeJobsBits(jobs);
  assert.deepStrictEqual(Array.from(e.jobOffsets), [0, 3, 4]);
  assert.deepStrictEqual(Array.from(e.src), [0xffffffff, 0, 1, 0, 0, 17, 13, 0, 0xffffffff, 1, 3, 0, 2, 0, 64, 2]);
  assert.deepStrictEqual(Array.from(e.bits), Array.from(bits13).concat(Array.from(bits64)));
  assert.deepStrictEqual(Array.from(e.pkIndices), [11, 5, 0x80000000, 3]);
  assert.deepStrictEqual(Array.from(e.rawPks.subarray(0, 96)), Array.from(raw));
  assert.deepStrictEqual(Array.from(e.sigLen), [96, 96, 192, 7]);
  assert.strictEqual(e.sigs[3 * 192], 0); // a signature of another length is not copied
  // what the batch stands for equals the explicit encoder's arrays for the same sets
  const plain = encodeJobs(jobs.map((j) => j.map((s) => explicitSet(s, lists))));
  const off = [0], idx = [];
  for (let i = 0; i < 4; i++) {
    const [list, o, len, bo] = Array.from(e.src.subarray(4 * i, 4 * i + 4));
    if (list === 0xffffffff) idx.push(...e.pkIndices.subarray(o, o + len));
    else idx.push(...intersectValues(e.bits.subarray(bo, bo + ((len + 7) >> 3)), len, Array.from(lists[list].subarray(o, o + len))));
    off.push(idx.length);
  }
  assert.deepStrictEqual(off, Array.from(plain.pkOffsets));
  assert.deepStrictEqual(idx, Array.from(plain.pkIndices));
  for (const k of ["jobOffsets", "msgs", "sigs", "sigLen"]) assert.deepStrictEqual(Array.from(e[k]), Array.from(plain[k]), k);
  // the routing rule: no committee set, no bits batch
  assert.strictEqual(hasCommitteeSets(jobs.map((j) => j.filter((s) => s.type !== "committee"))), false);
  // the caller-side checks
  const c = (over) => [Object.assign({type: "committee", committee: {list: 0, offset: 0, length: 9}, bits: Uint8Array.from([1, 1]),
    signingRoot: root(1), signature: sig(1)}, over)];
  checkSets(c({}));
  assert.throws(() => checkSets(c({bits: Uint8Array.from([1])})), /bitfield bytes/);
  assert.throws(() => checkSets(c({bits: Uint8Array.from([0, 0])})), /EMPTY_AGGREGATE_ARRAY/);
  assert.throws(() => checkSets(c({committee: {list: 8, offset: 0, length: 9}})), /list id/);
  assert.throws(() => checkSets(c({signingRoot: new Uint8Array(31)})), /32 bytes/);
  assert.throws(() => encodeJobsBits([c({bits: Uint8Array.from([1, 1, 1])})]), /bitfield bytes/);
  for (const k of ["verifyBits", "verifyBitsSync", "setIndexList", "indexListLen"]) assert.strictEqual(typeof addon[k], "function");
  for (const cls of [BlsGpuVerifier, BlsGpuSingleThreadVerifier]) assert.strictEqual(typeof cls.prototype.setIndexList, "function");
}

async function main() {
  hostChecks();
  if (process.argv[2] === "--host") {
    console.log("bits host checks OK");
    return;
  }
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const data = JSON.parse(fs.readFileSync(path.join(dir, "jobs.json")));
  const lists = {};
  for (const [id, v] of Object.entries(data.lists)) lists[id] = Uint32Array.from(v);
  const jobs = data.jobs.map((j) => j.map((s) => Object.assign(
    s.type === "committee" ? {type: "committee", committee: s.committee, bits: hex(s.bits)}
      : s.type === "single" ? {type: "single", pubkey: {index: s.indices[0]}}
        : {type: "aggregate", pubkeys: s.indices.map((index) => ({index}))},
    {signingRoot: hex(s.signingRoot), signature: hex(s.signature)})));
  const plainJobs = jobs.map((j) => j.map((s) => explicitSet(s, lists)));
  assert.strictEqual(jobs.reduce((a, j) => a + j.length, 0), 40);
  const nKeys = plainJobs.reduce((a, j) => a + j.reduce((b, s) => b + (s.type === "aggregate" ? s.pubkeys.length : 0), 0), 0);

  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
  try {
    v.pubkeysSet(0, table, 1);
    for (const [id, l] of Object.entries(lists)) v.setIndexList(Number(id), l);
    for (const c of v.allContexts()) for (const [id, l] of Object.entries(lists)) assert.strictEqual(addon.indexListLen(c, Number(id)), l.length);
    // committee sets and the explicit-index call on the same sets, job by job
    const got = await Promise.all(jobs.map((j) => v.verifySignatureSets(j, {batchable: true})));
    const want = await Promise.all(plainJobs.map((j) => v.verifySignatureSets(j, {batchable: true})));
    assert.deepStrictEqual(got, data.expected);
    assert.deepStrictEqual(want, data.expected);
    assert.strictEqual(v.metrics.lodestar_bls_aggregated_pubkeys_total, 2 * nKeys);
    // the priority context holds the lists too (verifyOnMainThread)
    for (const k of [0, data.bad_job]) {
      assert.strictEqual(await v.verifySignatureSets(jobs[k], {verifyOnMainThread: true}), data.expected[k]);
    }
    assert.strictEqual(v.verifySignatureSetsSync(jobs[1]), data.expected[1]);
    // the addon entries directly: sync and async agree with the explicit batch, counters included
    const eb = encodeJobsBits(jobs), ep = encodeJobs(plainJobs);
    const rs = addon.verifyBitsSync(v.ctx, eb);
    const ra = await addon.verifyBits(v.ctx, eb);
    const rp = addon.verifySync(v.ctx, ep);
    assert.deepStrictEqual(Array.from(rs.results), Array.from(rp.results));
    assert.deepStrictEqual(Array.from(ra.results), Array.from(rp.results));
    assert.deepStrictEqual(Array.from(rp.results), data.expected.map((x) => (x ? 1 : 0)));
    assert.strictEqual(rs.pubkeysAggregated, rp.pubkeysAggregated);
    assert.strictEqual(rs.batchRetries, 1);
    // refusals name the set; lengths come from the arrays
    const broken = Object.assign({}, eb, {src: Uint32Array.from(eb.src)});
    const k = Array.from({length: 40}, (_, i) => i).find((i) => broken.src[4 * i] !== 0xffffffff);
    broken.src[4 * k + 1] = 0xfffffff0;
    broken.src[4 * k + 2] = 0x20;
    assert.throws(() => addon.verifyBitsSync(v.ctx, broken), new RegExp(`bgv error -1: set ${k}:`));
    assert.throws(() => addon.verifyBitsSync(v.ctx, Object.assign({}, eb, {msgs: eb.msgs.subarray(0, 64)})), /shorter/);
    assert.throws(() => addon.verifyBitsSync(v.ctx, Object.assign({}, eb, {src: undefined})), /missing|wrong/);
    assert.throws(() => addon.verifyBitsSync(v.ctx, Object.assign({}, eb, {src: eb.src.subarray(0, 7)})), /four entries/);
    // a list entry with bit 31 is refused and the list stays; a dropped list refuses the sets that name it
    const id0 = Number(Object.keys(lists)[0]);
    assert.throws(() => v.setIndexList(id0, Uint32Array.from([1, 0x80000002])), /bit 31/);
    assert.strictEqual(addon.indexListLen(v.ctx, id0), lists[id0].length);
    v.setIndexList(id0, new Uint32Array(0));
    assert.strictEqual(addon.indexListLen(v.ctx, id0), 0);
    assert.throws(() => addon.verifyBitsSync(v.ctx, eb), /is not set/);
  } finally {
    await v.close();
  }

  const s = new BlsGpuSingleThreadVerifier({device: 0});
  try {
    s.pubkeysSet(0, table, 1);
    for (const [id, l] of Object.entries(lists)) s.setIndexList(Number(id), l);
    for (let k = 0; k < jobs.length; k++) {
      assert.strictEqual(await s.verifySignatureSets(jobs[k]), data.expected[k], `job ${k}`);
      assert.strictEqual(await s.verifySignatureSets(plainJobs[k]), data.expected[k], `plain job ${k}`);
    }
  } finally {
    await s.close();
  }
  console.log("bits test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
