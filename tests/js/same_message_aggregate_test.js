"use strict";
// GPU test of verifyAndAggregateSameMessage through the N-API addon
// (lodestar_amd/napi): two aggregate calls and one plain call with the same
// message in one flush; every aggregate call resolves with its own aggregate,
// byte for byte what tests/test_napi_same_message_aggregate.py computed with
// the Python oracle (argv[2]: table96.bin and calls.json).  Exits non-zero on
// any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeSameMessage, mergeSameMessage, encodeAggregateSide, G2_IDENTITY_96} =
  require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));
const toHex = (b) => Buffer.from(b).toString("hex");

async function main() {
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const doc = JSON.parse(fs.readFileSync(path.join(dir, "calls.json")));
  const message = hex(doc.message);
  const calls = doc.calls.map((c) => ({
    message, expected: c.expected, aggregate: c.aggregate, count: c.count,
    agg: c.plain ? undefined : {previous: c.previous ? hex(c.previous) : null, take: c.take != null ? c.take : null},
    sets: c.sets.map((s) => ({publicKey: {index: s.index}, signature: hex(s.signature)})),
  }));

  // the merge rule without a device: an aggregate call always forms its own group
  const merged = mergeSameMessage(calls);
  assert.strictEqual(merged.groups.length, calls.length);
  assert.deepStrictEqual(merged.groupOf, calls.map((_, k) => k));
  const plainTwice = mergeSameMessage([calls[2], calls[2], calls[0]]);
  assert.deepStrictEqual(plainTwice.groupOf, [0, 0, 1]);
  const n = calls.reduce((a, c) => a + c.sets.length, 0);
  const side = encodeAggregateSide(calls, merged, n);
  assert.strictEqual(side.take.length, n);
  assert.deepStrictEqual(Array.from(side.take.subarray(merged.where[2][0], merged.where[2][1])), calls[2].sets.map(() => 0));
  assert.strictEqual(toHex(side.prevSigs.subarray(0, 96)), toHex(G2_IDENTITY_96));
  assert.strictEqual(toHex(side.prevSigs.subarray(96, 192)), toHex(calls[1].agg.previous));

  const run = (v, c, batchable) => (c.agg
    ? v.verifyAndAggregateSameMessage(c.sets, c.message, {batchable, previous: c.agg.previous != null ? c.agg.previous : undefined, take: c.agg.take != null ? c.agg.take : undefined})
    : v.verifySignatureSetsSameMessage(c.sets, c.message, {batchable}));
  const check = (r, c, label) => {
    if (!c.agg) return assert.deepStrictEqual(r, c.expected, label);
    assert.deepStrictEqual(r.valid, c.expected, label);
    assert.strictEqual(toHex(r.aggregate), c.aggregate, label);
    assert.strictEqual(r.count, c.count, label);
  };

  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
  try {
    v.pubkeysSet(0, table, 1);
    const results = await Promise.all(calls.map((c) => run(v, c, true)));
    results.forEach((r, k) => check(r, calls[k], `call ${k}`));
    assert.strictEqual(v.smDeviceCalls, 1, "one flush, one merged device call");
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_sig_sets_started_total, n);
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_aggregated_sigs_total, calls[0].count + calls[1].count);
    // a previous that does not decode rejects that call alone
    const bad = new Uint8Array(96).fill(0xff);
    bad[0] = 0x9f;
    const settled = await Promise.allSettled([
      v.verifyAndAggregateSameMessage(calls[0].sets, message, {batchable: true, previous: bad}),
      run(v, calls[1], true), run(v, calls[2], true)]);
    assert.strictEqual(settled[0].status, "rejected");
    assert.match(String(settled[0].reason.message), /^BLST_ERROR: BLST_BAD_ENCODING$/);
    check(settled[1].value, calls[1], "beside a rejected call");
    check(settled[2].value, calls[2], "beside a rejected call");
    await assert.rejects(v.verifyAndAggregateSameMessage(calls[0].sets, message, {previous: new Uint8Array(95)}), /BLST_INVALID_SIZE/);
    const empty = await v.verifyAndAggregateSameMessage([], message);
    assert.deepStrictEqual(empty.valid, []);
    assert.strictEqual(toHex(empty.aggregate), toHex(G2_IDENTITY_96));
    // the addon entry points directly: sync and async agree; take and prevSigs are optional
    const one = encodeSameMessage([{message, sets: calls[0].sets}]);
    const rs = addon.verifySameMessageAggregateSync(v.ctx, one);
    const ra = await addon.verifySameMessageAggregate(v.ctx, one);
    assert.strictEqual(toHex(rs.aggSigs), calls[0].aggregate);
    assert.strictEqual(toHex(ra.aggSigs), calls[0].aggregate);
    assert.deepStrictEqual(Array.from(rs.aggCount), [calls[0].count]);
    assert.deepStrictEqual(Array.from(rs.aggCode), [0]);
    assert.deepStrictEqual(Array.from(rs.valid), Array.from(addon.verifySameMessageSync(v.ctx, one).valid));
    assert.throws(() => addon.verifySameMessageAggregateSync(v.ctx, {...one, take: new Uint8Array(1)}), RangeError);
  } finally {
    await v.close();
  }
  await assert.rejects(v.verifyAndAggregateSameMessage(calls[0].sets, message), /QUEUE_ERROR_QUEUE_ABORTED/);

  const s = new BlsGpuSingleThreadVerifier({device: 0});
  try {
    s.pubkeysSet(0, table, 1);
    check(await run(s, calls[1], false), calls[1], "single thread");
  } finally {
    await s.close();
  }
  console.log("same message aggregate test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
