"use strict";
// verifyAggregateSetsSameMessage through the N-API addon (lodestar_amd/napi).
//   node same_message_agg_test.js --host   the encoder and the merge rule, no device
//   node same_message_agg_test.js DIR      those, then on the GPU: three calls at once, two batchable
//                                          and one not, with one bad signature in one of them
// The signed calls come from tests/test_napi_same_message_agg.py (DIR: table96.bin
// and calls.json).  Exits non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeSameMessageAgg, encodeSameMessage, mergeSameMessage,
  checkAggregateSameMessage} = require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

function hostChecks() {
  const m1 = new Uint8Array(32).fill(1), m2 = new Uint8Array(32).fill(2);
  const raw = Uint8Array.from({length: 96}, (_, k) => k);
  const sig = (b, n = 96) => new Uint8Array(n).fill(b);
  const calls = [
    {message: m1, sets: [{publicKeys: [{index: 3}, {index: 7}], signature: sig(0xaa)}, {publicKeys: [4], signature: sig(0xbb, 192)}]},
    {message: m2, sets: [{publicKeys: [{raw}, 1, {raw}], signature: sig(0xcc)}]},
    {message: m1, sets: [{publicKeys: Uint32Array.from([9, 8, 7, 6]), signature: sig(0xdd, 7)}]},
  ];
  // one group per call, calls with byte-equal messages share a group (first appearance order)
  const {groups, where} = mergeSameMessage(calls);
  assert.strictEqual(groups.length, 2);
  assert.deepStrictEqual(where, [[0, 2], [3, 4], [2, 3]]);
  const enc = encodeSameMessageAgg(groups);
  assert.deepStrictEqual(Array.from(enc.groupOffsets), [0, 3, 4]);
  assert.deepStrictEqual(Array.from(enc.pkOffsets), [0, 2, 3, 7, 10]);
  assert.deepStrictEqual(Array.from(enc.pkIndices), [3, 7, 4, 9, 8, 7, 6, 0x80000000, 1, 0x80000001]);
  assert.deepStrictEqual(Array.from(enc.rawPks.subarray(0, 96)), Array.from(raw));
  assert.deepStrictEqual(Array.from(enc.sigLen), [96, 192, 7, 96]);
  assert.strictEqual(enc.msgs.length, 64);
  assert.strictEqual(enc.msgs[0], 1);
  assert.strictEqual(enc.msgs[32], 2);
  assert.strictEqual(enc.sigs[192], 0xbb);
  assert.strictEqual(enc.sigs[192 + 191], 0xbb);
  assert.strictEqual(enc.sigs[2 * 192], 0); // a signature of another length is not copied
  // single-key sets encode as the single-key entry does
  const single = [{message: m1, sets: [{publicKey: {index: 5}, signature: sig(1)}, {publicKey: {index: 6}, signature: sig(2)}]}];
  const a1 = encodeSameMessage(single);
  const aA = encodeSameMessageAgg(single.map((g) => ({message: g.message, sets: g.sets.map((s) => ({publicKeys: [s.publicKey], signature: s.signature}))})));
  assert.deepStrictEqual(Array.from(aA.pkOffsets), [0, 1, 2]);
  for (const k of ["groupOffsets", "pkIndices", "msgs", "sigs", "sigLen"]) assert.deepStrictEqual(Array.from(aA[k]), Array.from(a1[k]), k);
  // the caller-side checks
  assert.throws(() => checkAggregateSameMessage([{publicKeys: [], signature: sig(1)}], m1), /EMPTY_AGGREGATE_ARRAY/);
  assert.throws(() => checkAggregateSameMessage([{signature: sig(1)}], m1), /EMPTY_AGGREGATE_ARRAY/);
  assert.throws(() => checkAggregateSameMessage([{publicKeys: [{raw: new Uint8Array(48)}], signature: sig(1)}], m1), /96-byte/);
  assert.throws(() => checkAggregateSameMessage([{publicKeys: [1], signature: sig(1)}], new Uint8Array(31)), /32 bytes/);
  assert.throws(() => encodeSameMessageAgg([{message: m1, sets: []}]), /Empty signature set/);
  checkAggregateSameMessage(calls[1].sets, m2);
  for (const k of ["verifySameMessageAgg", "verifySameMessageAggSync"]) assert.strictEqual(typeof addon[k], "function");
}

async function main() {
  hostChecks();
  if (process.argv[2] === "--host") {
    console.log("same message agg host checks OK");
    return;
  }
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const calls = JSON.parse(fs.readFileSync(path.join(dir, "calls.json"))).map((c, k) => ({
    message: hex(c.message), batchable: c.batchable, expected: c.expected,
    // keys as validator indices in one call, as {index} objects in the others
    sets: c.sets.map((s) => ({publicKeys: k === 1 ? s.indices : s.indices.map((i) => ({index: i})), signature: hex(s.signature)})),
  }));
  const n = calls.reduce((a, c) => a + c.sets.length, 0);
  const nKeys = calls.reduce((a, c) => a + c.sets.reduce((b, s) => b + s.publicKeys.length, 0), 0);

  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
  try {
    v.pubkeysSet(0, table, 1);
    assert.strictEqual(v.canAcceptWork(), true);
    const results = await Promise.all(calls.map((c) => v.verifyAggregateSetsSameMessage(c.sets, c.message, {batchable: c.batchable})));
    results.forEach((r, k) => assert.deepStrictEqual(r, calls[k].expected, `call ${k}`));
    assert.ok(v.smaDeviceCalls >= 1 && v.smaDeviceCalls <= 2, `device calls ${v.smaDeviceCalls}`);
    assert.strictEqual(v.smDeviceCalls, 0); // the single-key buffer is not involved
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_agg_sig_sets_started_total, n);
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_agg_retries_total, 1);
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_sig_sets_started_total, 0);
    assert.strictEqual(v.metrics.lodestar_bls_aggregated_pubkeys_total, nKeys);
    assert.deepStrictEqual(await v.verifyAggregateSetsSameMessage([], calls[0].message), []);
    // the addon entry points directly: sync and async agree, and name the retried group
    const one = encodeSameMessageAgg([{message: calls[1].message, sets: calls[1].sets}]);
    const rs = addon.verifySameMessageAggSync(v.ctx, one);
    const ra = await addon.verifySameMessageAgg(v.ctx, one);
    assert.deepStrictEqual(Array.from(rs.valid, (x) => x === 1), calls[1].expected);
    assert.deepStrictEqual(Array.from(ra.valid), Array.from(rs.valid));
    assert.strictEqual(rs.groupsRetried, 1);
    assert.strictEqual(rs.hashes, 1);
    assert.ok(rs.pairs <= 2 * rs.segments);
    // lengths are checked against the copied offsets
    assert.throws(() => addon.verifySameMessageAggSync(v.ctx, Object.assign({}, one, {pkIndices: one.pkIndices.subarray(0, 3)})), /shorter/);
    assert.throws(() => addon.verifySameMessageAggSync(v.ctx, Object.assign({}, one, {pkOffsets: undefined})), /missing|wrong/);
  } finally {
    await v.close();
  }
  await assert.rejects(v.verifyAggregateSetsSameMessage(calls[0].sets, calls[0].message), /QUEUE_ERROR_QUEUE_ABORTED/);

  const s = new BlsGpuSingleThreadVerifier({device: 0});
  try {
    s.pubkeysSet(0, table, 1);
    assert.deepStrictEqual(await s.verifyAggregateSetsSameMessage(calls[1].sets, calls[1].message), calls[1].expected);
    assert.strictEqual(s.metrics.lodestar_bls_aggregated_pubkeys_total, calls[1].sets.reduce((b, x) => b + x.publicKeys.length, 0));
  } finally {
    await s.close();
  }
  console.log("same message agg test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
