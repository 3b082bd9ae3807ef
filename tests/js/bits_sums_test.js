"use strict";
// Committee sets over index lists with resident prefix sums ({sums: true}) through the N-API addon.
//   node bits_sums_test.js --host   the new entries exist
//   node bits_sums_test.js DIR      on the GPU: one committee batch through a verifier with sums and one without; the
//                                   verdicts agree and bitsPathStats shows the complement path on the first only
// The signed jobs come from tests/test_napi_bits_sums.py (DIR: table96.bin and jobs.json).  Exits non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeJobsBits} = require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

function hostChecks() {
  for (const k of ["setIndexListSums", "indexListHasSums", "bitsPathStats"]) assert.strictEqual(typeof addon[k], "function", k);
  for (const cls of [BlsGpuVerifier, BlsGpuSingleThreadVerifier]) assert.strictEqual(cls.prototype.setIndexList.length, 2);
}

async function main() {
  hostChecks();
  if (process.argv[2] === "--host") {
    console.log("bits sums host checks OK");
    return;
  }
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const data = JSON.parse(fs.readFileSync(path.join(dir, "jobs.json")));
  const lists = {};
  for (const [id, v] of Object.entries(data.lists)) lists[id] = Uint32Array.from(v);
  const jobs = data.jobs.map((j) => j.map((s) => ({type: "committee", committee: s.committee, bits: hex(s.bits),
    signingRoot: hex(s.signingRoot), signature: hex(s.signature)})));
  const eb = encodeJobsBits(jobs);
  const stats = {};
  const verdicts = {};
  for (const sums of [true, false]) {
    const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
    try {
      v.pubkeysSet(0, table, 1);
      for (const [id, l] of Object.entries(lists)) v.setIndexList(Number(id), l, {sums});
      for (const c of v.allContexts()) for (const id of Object.keys(lists)) assert.strictEqual(addon.indexListHasSums(c, Number(id)), sums);
      verdicts[sums] = await Promise.all(jobs.map((j) => v.verifySignatureSets(j, {batchable: true})));
      // the priority context holds the sums too
      assert.strictEqual(await v.verifySignatureSets(jobs[0], {verifyOnMainThread: true}), data.expected[0]);
      const r = addon.verifyBitsSync(v.ctx, eb);
      assert.deepStrictEqual(Array.from(r.results), data.expected.map((x) => (x ? 1 : 0)));
      stats[sums] = addon.bitsPathStats(v.ctx);
      assert.strictEqual(r.pubkeysAggregated, stats[sums].keysExpanded);
      if (sums) {  // a rewritten row drops the sums of every list; dropping on request works too
        v.pubkeysSet(0, table.subarray(0, 96), 1);
        for (const c of v.allContexts()) for (const id of Object.keys(lists)) assert.strictEqual(addon.indexListHasSums(c, Number(id)), false);
        assert.throws(() => addon.setIndexListSums(v.ctx, 7, true), /bgv error -1/);
      }
    } finally {
      await v.close();
    }
  }
  assert.deepStrictEqual(verdicts[true], data.expected);
  assert.deepStrictEqual(verdicts[false], data.expected);
  assert.strictEqual(stats[true].setsComplement, data.n_complement);
  assert.ok(stats[true].setsComplement > 0 && stats[true].keysGathered < stats[true].keysExpanded);
  assert.strictEqual(stats[false].setsComplement, 0);
  assert.strictEqual(stats[false].keysGathered, stats[false].keysExpanded);
  assert.strictEqual(stats[true].keysExpanded, stats[false].keysExpanded);

  const s = new BlsGpuSingleThreadVerifier({device: 0});
  try {
    s.pubkeysSet(0, table, 1);
    for (const [id, l] of Object.entries(lists)) s.setIndexList(Number(id), l, {sums: true});
    for (let k = 0; k < jobs.length; k++) assert.strictEqual(await s.verifySignatureSets(jobs[k]), data.expected[k], `job ${k}`);
    assert.ok(addon.bitsPathStats(s.ctx).setsComplement > 0);
  } finally {
    await s.close();
  }
  console.log("bits sums test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
