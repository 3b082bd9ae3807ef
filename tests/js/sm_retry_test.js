"use strict";
// GPU test of the split retry of the same-message entries through the N-API
// addon (lodestar_amd/napi): smRetry / smRetryStats on a context, and the
// smRetry option and sm_retry_* counters of both pools.  One call of 64 sets
// with one bad signature: the per-set retry decides 64 sets on their own, the
// split retry 8 subs and 8 leaves.  The signed call comes from
// tests/test_napi_sm_retry.py (argv[2]: table96.bin and call.json).  Exits
// non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeSameMessage} =
  require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

const SPLIT = {mode: 1, segments: 1, subs: 8, subsFailed: 1, leaves: 8, pairs: 32, hashes: 0};
const PER_SET = {mode: 0, segments: 1, subs: 0, subsFailed: 0, leaves: 64, pairs: 128, hashes: 64};

async function main() {
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const c = JSON.parse(fs.readFileSync(path.join(dir, "call.json")));
  const message = hex(c.message);
  const sets = c.sets.map((s) => ({publicKey: {index: s.index}, signature: hex(s.signature)}));

  for (const smRetry of [false, true]) {
    const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1, smRetry});
    try {
      v.pubkeysSet(0, table, 1);
      assert.strictEqual(v.smRetry, smRetry);
      assert.deepStrictEqual(await v.verifySignatureSetsSameMessage(sets, message), c.expected);
      const want = smRetry ? SPLIT : PER_SET;
      assert.strictEqual(v.metrics.sm_retry_subs, want.subs);
      assert.strictEqual(v.metrics.sm_retry_leaves, want.leaves);
      assert.strictEqual(v.metrics.sm_retry_pairs, want.pairs);
      assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_retries_total, 1);
      assert.deepStrictEqual(addon.smRetryStats(v.ctx), want);
      if (smRetry) continue;
      // the addon entry points directly, switching the context between calls
      const one = encodeSameMessage([{message, sets}]);
      for (const [mode, path_] of [[1, SPLIT], [0, PER_SET], [true, SPLIT], [false, PER_SET]]) {
        addon.smRetry(v.ctx, mode);
        const r = addon.verifySameMessageSync(v.ctx, one);
        assert.deepStrictEqual(Array.from(r.valid, (x) => x === 1), c.expected);
        assert.strictEqual(r.setsRetried, 64);
        assert.deepStrictEqual(addon.smRetryStats(v.ctx), path_);
      }
      assert.throws(() => addon.smRetry(v.ctx, 2), /bgv_sm_retry mode 2/);
      assert.throws(() => addon.smRetry(v.ctx, -1), /bgv_sm_retry mode -1/);
    } finally {
      await v.close();
    }
  }

  const s = new BlsGpuSingleThreadVerifier({device: 0, smRetry: true});
  try {
    s.pubkeysSet(0, table, 1);
    assert.deepStrictEqual(await s.verifySignatureSetsSameMessage(sets, message), c.expected);
    assert.deepStrictEqual(addon.smRetryStats(s.ctx), SPLIT);
  } finally {
    await s.close();
  }
  console.log("sm retry test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
