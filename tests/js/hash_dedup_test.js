"use strict";
// hash_to_G2 once per distinct signing root (bgv_cfg.hash_dedup) through the N-API addon.
//   node hash_dedup_test.js DIR   on the GPU: a 256-set, 4-job batch with 16 distinct roots through addon.verify on a
//                                 context opened in the bulk layout with the grouping on ({split: 0, hashDedup: 1}; the
//                                 pool chooses the layout by batch size and cannot force it), through contexts that
//                                 hash every set (auto, {hashDedup: 0}, the latency layout), and through the pool
// The signed jobs come from tests/test_napi_hash_dedup.py (DIR: table96.bin and jobs.json).  Exits non-zero on any mismatch.
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
  assert.throws(() => addon.open(0, 0, {hashDedup: 2}), /bgv error -1/);
  assert.throws(() => addon.open(0, 0, {lanes: 1}), /cfg takes/);
  for (const [cfg, hashes, dedup] of [[{split: 0, hashDedup: 1}, 16, 1], [{split: 0}, 256, 0], [{split: 0, hashDedup: 0}, 256, 0],
    [{split: 1, hashDedup: 1}, 256, 0]]) {
    const ctx = addon.open(0, 0, cfg);
    try {
      addon.pubkeysSet(ctx, 0, table, 1);
      const r = await addon.verify(ctx, batch);
      assert.deepStrictEqual(Array.from(r.results), want, JSON.stringify(cfg));
      assert.strictEqual(r.hashes, hashes, JSON.stringify(cfg));
      assert.deepStrictEqual(addon.hashStats(ctx), {sets: nSets, hashes, dedup});
      const s = addon.verifySync(ctx, batch);
      assert.deepStrictEqual(Array.from(s.results), want);
      assert.strictEqual(s.hashes, hashes);
      const p = await addon.partial(ctx, batch);
      assert.strictEqual(p.hashes, hashes);
    } finally {
      addon.close(ctx);
    }
  }
  // the pool: its two counters per device batch (256 sets take the latency layout there: one evaluation per set)
  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
  try {
    v.pubkeysSet(0, table, 1);
    assert.strictEqual(v.metrics.hashToG2Sets, undefined);
    const verdicts = await Promise.all(jobs.map((j) => v.verifySignatureSets(j, {batchable: true})));
    assert.deepStrictEqual(verdicts, data.expected);
    assert.strictEqual(v.metrics.hashToG2Sets, nSets);
    assert.strictEqual(v.metrics.hashToG2Evaluated, nSets);
  } finally {
    await v.close();
  }
  console.log("hash dedup test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
