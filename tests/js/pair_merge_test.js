"use strict";
// One Miller pair per distinct signing root of a job (bgv_pair_merge) through the N-API addon.
//   node pair_merge_test.js DIR   on the GPU: a 256-set, 4-job batch with 16 distinct roots through addon.verify,
//                                 verifySync and partial on a context in the layout that merges ({split: 0, miller: 1};
//                                 the pool chooses the layout by batch size and cannot force it) with pairMerge on and
//                                 off, through a latency-layout context with it on, and through the pool
// The signed jobs come from tests/test_napi_pair_merge.py (DIR: table96.bin and jobs.json).  Exits non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, encodeJobs} = require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

async function main() {
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const data = JSON.parse(fs.readFileSync(path.join(dir, "jobs.json")));
  const jobs = data.jobs.map((j) => j.map((s) => ({type: "aggregate", pubkeys: s.indices.map((index) => ({index})),
    signingRoot: hex(s.signingRoot), signature: hex(s.signature)})));
  const want = data.expected.map((x) => (x ? 1 : 0));
  const batch = encodeJobs(jobs);
  const nSets = batch.pkOffsets.length - 1;
  assert.strictEqual(nSets, 256);
  assert.ok(data.pairs < nSets);
  assert.strictEqual(typeof addon.pairMerge, "function");
  assert.strictEqual(typeof addon.pairStats, "function");
  for (const [cfg, on, pairs, merged] of [[{split: 0, miller: 1}, true, data.pairs, 1], [{split: 0, miller: 1}, false, nSets, 0],
    [{split: 1}, true, nSets, 0]]) {
    const ctx = addon.open(0, 0, cfg);
    try {
      addon.pubkeysSet(ctx, 0, table, 1);
      assert.deepStrictEqual(addon.pairStats(ctx), {sets: 0, pairs: 0, merged: 0, fallback: 0});
      assert.throws(() => addon.pairMerge(ctx, 2), /bgv error -1/);
      addon.pairMerge(ctx, on);
      const r = await addon.verify(ctx, batch);
      assert.deepStrictEqual(Array.from(r.results), want, JSON.stringify(cfg));
      assert.strictEqual(r.millerPairs, pairs, JSON.stringify(cfg));
      assert.deepStrictEqual(addon.pairStats(ctx), {sets: nSets, pairs, merged, fallback: 0});
      const s = addon.verifySync(ctx, batch);
      assert.deepStrictEqual(Array.from(s.results), want);
      assert.strictEqual(s.millerPairs, pairs);
      const p = await addon.partial(ctx, batch);
      assert.strictEqual(p.millerPairs, pairs);
      assert.strictEqual(addon.pairStats(ctx).merged, merged);
      addon.pairMerge(ctx, 0); // from the next call on
      const off = await addon.verify(ctx, batch);
      assert.deepStrictEqual(Array.from(off.results), want);
      assert.strictEqual(off.millerPairs, nSets);
    } finally {
      addon.close(ctx);
    }
  }
  // the pool: the option reaches its bulk contexts and the two counters appear with the first batch (256 sets take
  // the latency layout there: one pair per set)
  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1, pairMerge: true});
  try {
    v.pubkeysSet(0, table, 1);
    assert.strictEqual(v.pairMerge, true);
    assert.strictEqual(v.metrics.millerPairsSets, undefined);
    const verdicts = await Promise.all(jobs.map((j) => v.verifySignatureSets(j, {batchable: true})));
    assert.deepStrictEqual(verdicts, data.expected);
    assert.strictEqual(v.metrics.millerPairsSets, nSets);
    assert.strictEqual(v.metrics.millerPairsEvaluated, nSets);
  } finally {
    await v.close();
  }
  console.log("pair merge test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
