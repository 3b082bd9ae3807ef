"use strict";
// GPU test of verifySignatureSetsSameMessage through the N-API addon
// (lodestar_amd/napi): three calls at once, two batchable and one not, with
// one bad signature in one of them; the results are per call and per set.
// The signed calls come from tests/test_napi_same_message.py (argv[2]:
// table96.bin and calls.json).  Exits non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeSameMessage, mergeSameMessage} =
  require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

async function main() {
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const calls = JSON.parse(fs.readFileSync(path.join(dir, "calls.json"))).map((c) => ({
    message: hex(c.message), batchable: c.batchable, expected: c.expected,
    sets: c.sets.map((s) => ({publicKey: {index: s.index}, signature: hex(s.signature)})),
  }));

  // the merge rule without a device: one group per call, equal messages share a group
  const {groups, where} = mergeSameMessage(calls);
  assert.strictEqual(groups.length, 2);
  assert.deepStrictEqual(where.map((w) => w[1] - w[0]), calls.map((c) => c.sets.length));
  const enc = encodeSameMessage(groups);
  assert.deepStrictEqual(Array.from(enc.groupOffsets), [0, groups[0].sets.length, groups[0].sets.length + groups[1].sets.length]);

  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
  try {
    v.pubkeysSet(0, table, 1);
    assert.strictEqual(v.canAcceptWork(), true);
    const results = await Promise.all(calls.map((c) => v.verifySignatureSetsSameMessage(c.sets, c.message, {batchable: c.batchable})));
    results.forEach((r, k) => assert.deepStrictEqual(r, calls[k].expected, `call ${k}`));
    assert.ok(v.smDeviceCalls >= 1 && v.smDeviceCalls <= 2, `device calls ${v.smDeviceCalls}`);
    const n = calls.reduce((a, c) => a + c.sets.length, 0);
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_sig_sets_started_total, n);
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_retries_total, 1);
    assert.deepStrictEqual(await v.verifySignatureSetsSameMessage([], calls[0].message), []);
    // the addon entry points directly: sync and async agree, and name the retried group
    const one = encodeSameMessage([{message: calls[1].message, sets: calls[1].sets}]);
    const rs = addon.verifySameMessageSync(v.ctx, one);
    const ra = await addon.verifySameMessage(v.ctx, one);
    assert.deepStrictEqual(Array.from(rs.valid, (x) => x === 1), calls[1].expected);
    assert.deepStrictEqual(Array.from(ra.valid), Array.from(rs.valid));
    assert.strictEqual(rs.groupsRetried, 1);
    assert.strictEqual(rs.hashes, 1);
    assert.ok(rs.pairs <= 2 * rs.segments);
  } finally {
    await v.close();
  }
  await assert.rejects(v.verifySignatureSetsSameMessage(calls[0].sets, calls[0].message), /QUEUE_ERROR_QUEUE_ABORTED/);

  const s = new BlsGpuSingleThreadVerifier({device: 0});
  try {
    s.pubkeysSet(0, table, 1);
    assert.deepStrictEqual(await s.verifySignatureSetsSameMessage(calls[1].sets, calls[1].message), calls[1].expected);
  } finally {
    await s.close();
  }
  console.log("same message test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
