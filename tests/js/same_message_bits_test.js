"use strict";
// Committee sets in verifyAggregateSetsSameMessage through the N-API addon (lodestar_amd/napi).
//   node same_message_bits_test.js --host DIR   encodeSameMessageBits against the Python encoder's arrays
//                                               (DIR/want.json) and the caller-side checks, no device
//   node same_message_bits_test.js DIR          on the GPU: a mixed call of committee and explicit sets through
//                                               both classes with the key metric, then a call without committee
//                                               sets, which takes the old path
// The signed calls come from tests/test_napi_same_message_bits.py (DIR: table96.bin, list.json, calls.json).
// Exits non-zero on any mismatch.
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const {addon, BlsGpuVerifier, BlsGpuSingleThreadVerifier, encodeSameMessageBits, encodeSameMessageAgg, hasCommitteeKeys,
  mergeSameMessage, checkAggregateSameMessage} = require(path.join(__dirname, "..", "..", "lodestar_amd", "napi"));
const hex = (s) => Uint8Array.from(Buffer.from(s, "hex"));

function hostChecks(dir) {
  const m1 = new Uint8Array(32).fill(1), m2 = new Uint8Array(32).fill(2);
  const raw = Uint8Array.from({length: 96}, (_, k) => k);
  const sig = (b, n = 96) => new Uint8Array(n).fill(b);
  const ones = (n, last) => { const b = new Uint8Array(n).fill(0xff); b[n - 1] = last; return b; };
  // the groups of tests/test_same_message_bits_host.py
  const groups = [
    {message: m1, sets: [
      {committee: {list: 0, offset: 64, length: 128}, bits: ones(16, 0x7f), signature: sig(0xa1)},
      {publicKeys: [{index: 5}, {raw}, {index: 3}], signature: sig(0xa2, 192)},
      {committee: {list: 1, offset: 1, length: 13}, bits: Uint8Array.from([0xb5, 0x12]), signature: sig(0xa3, 7)}]},
    {message: m2, sets: [
      {publicKeys: [9, 8], signature: sig(0xa4)},
      {committee: {list: 1, offset: 0, length: 512}, bits: ones(64, 0xff), signature: sig(0xa5)},
      {publicKeys: [{raw}], signature: sig(0xa6)}]},
  ];
  assert.strictEqual(hasCommitteeKeys(groups), true);
  const enc = encodeSameMessageBits(groups);
  const want = JSON.parse(fs.readFileSync(path.join(dir, "want.json")));
  for (const k of ["groupOffsets", "src", "bits", "msgs", "sigs", "sigLen"]) assert.deepStrictEqual(Array.from(enc[k]), want[k], k);
  // the JavaScript encoder stores a raw key once per use, the Python one once per distinct key: the keys are equal
  assert.deepStrictEqual(Array.from(enc.pkIndices), [5, 0x80000000, 3, 9, 8, 0x80000001]);
  assert.deepStrictEqual(Array.from(enc.rawPks.subarray(0, 96)), want.rawPks);
  assert.deepStrictEqual(Array.from(enc.rawPks.subarray(96, 192)), want.rawPks);
  assert.strictEqual(enc.src.length, 4 * 6);
  // a call without committee sets keeps the old encoder
  const plain = groups.map((g) => ({message: g.message, sets: g.sets.filter((s) => !s.committee)}));
  assert.strictEqual(hasCommitteeKeys(plain), false);
  const b = encodeSameMessageBits(plain), e = encodeSameMessageAgg(plain);
  assert.deepStrictEqual(Array.from(b.pkIndices), Array.from(e.pkIndices).slice(0, b.pkIndices.length));
  assert.deepStrictEqual(Array.from(b.src).filter((_, k) => k % 4 === 1), Array.from(e.pkOffsets).slice(0, -1));
  assert.strictEqual(b.bits.length, 0);
  // the caller-side checks of committee sets
  const ok = {committee: {list: 0, offset: 0, length: 9}, bits: Uint8Array.from([1, 1]), signature: sig(1)};
  checkAggregateSameMessage([ok, {publicKeys: [1], signature: sig(1)}], m1);
  const bad = [
    Object.assign({}, ok, {bits: Uint8Array.from([1])}),
    Object.assign({}, ok, {bits: Uint8Array.from([1, 0, 0])}),
    Object.assign({}, ok, {committee: {list: 8, offset: 0, length: 9}}),
    Object.assign({}, ok, {bits: undefined}),
  ];
  for (const s of bad) assert.throws(() => checkAggregateSameMessage([ok, s], m1), /committee set/);
  assert.throws(() => checkAggregateSameMessage([Object.assign({}, ok, {bits: Uint8Array.from([0, 0])})], m1), /EMPTY_AGGREGATE_ARRAY/);
  assert.throws(() => checkAggregateSameMessage([ok], new Uint8Array(31)), /32 bytes/);
  assert.throws(() => encodeSameMessageBits([{message: m1, sets: []}]), /Empty signature set/);
  for (const k of ["verifySameMessageBits", "verifySameMessageBitsSync"]) assert.strictEqual(typeof addon[k], "function");
}

async function main() {
  if (process.argv[2] === "--host") {
    hostChecks(process.argv[3]);
    console.log("same message bits host checks OK");
    return;
  }
  const dir = process.argv[2];
  const table = new Uint8Array(fs.readFileSync(path.join(dir, "table96.bin")));
  const list = Uint32Array.from(JSON.parse(fs.readFileSync(path.join(dir, "list.json"))));
  const data = JSON.parse(fs.readFileSync(path.join(dir, "calls.json")));
  const toSet = (s) => (s.committee
    ? {committee: s.committee, bits: hex(s.bits), signature: hex(s.signature)}
    : {publicKeys: s.indices, signature: hex(s.signature)});
  const calls = data.calls.map((c) => ({message: hex(c.message), batchable: c.batchable, expected: c.expected, keys: c.keys,
    sets: c.sets.map(toSet)}));
  const mixed = calls.slice(0, 2), plain = calls[2];
  const mixedKeys = mixed.reduce((a, c) => a + c.keys, 0);

  const v = new BlsGpuVerifier({device: 0, contextsPerDevice: 1});
  try {
    v.pubkeysSet(0, table, 1);
    v.setIndexList(data.listId, list, {sums: true});
    const results = await Promise.all(mixed.map((c) => v.verifyAggregateSetsSameMessage(c.sets, c.message, {batchable: c.batchable})));
    results.forEach((r, k) => assert.deepStrictEqual(r, mixed[k].expected, `call ${k}`));
    assert.strictEqual(v.smaDeviceCalls, 1); // merged: more than 32 buffered signatures flush the buffer
    assert.strictEqual(v.metrics.lodestar_bls_aggregated_pubkeys_total, mixedKeys); // from the device's path counters
    assert.strictEqual(v.metrics.lodestar_bls_thread_pool_same_message_agg_retries_total, 1);
    const ps = addon.bitsPathStats(v.ctxs[0]);
    assert.strictEqual(ps.keysExpanded, mixedKeys);
    assert.ok(ps.setsComplement > 0 && ps.keysGathered < ps.keysExpanded);
    // a call without committee sets: the old path, the key count from pkOffsets, the path counters untouched
    assert.deepStrictEqual(await v.verifyAggregateSetsSameMessage(plain.sets, plain.message), plain.expected);
    assert.strictEqual(v.metrics.lodestar_bls_aggregated_pubkeys_total, mixedKeys + plain.keys);
    assert.strictEqual(addon.bitsPathStats(v.ctxs[0]).keysExpanded, mixedKeys);
    // the addon entry points directly: sync and async agree
    const {groups} = mergeSameMessage(mixed);
    const one = encodeSameMessageBits(groups);
    const rs = addon.verifySameMessageBitsSync(v.ctxs[0], one);
    const ra = await addon.verifySameMessageBits(v.ctxs[0], one);
    assert.deepStrictEqual(Array.from(ra.valid), Array.from(rs.valid));
    assert.strictEqual(rs.valid.reduce((a, x) => a + (x === 1 ? 0 : 1), 0), 1);
    assert.strictEqual(rs.pubkeysAggregated, mixedKeys);
    assert.strictEqual(rs.groupsRetried, 1);
    assert.strictEqual(rs.hashes, groups.length);
    // lengths are checked against the copies taken at call time
    assert.throws(() => addon.verifySameMessageBitsSync(v.ctxs[0], Object.assign({}, one, {sigLen: one.sigLen.subarray(0, 3)})), /shorter/);
    assert.throws(() => addon.verifySameMessageBitsSync(v.ctxs[0], Object.assign({}, one, {src: one.src.subarray(0, 8)})), /groupOffsets/);
    assert.throws(() => addon.verifySameMessageBitsSync(v.ctxs[0], Object.assign({}, one, {bits: undefined})), /missing|wrong/);
    // the library's refusals name the set
    const src = Uint32Array.from(one.src);
    const k = Array.from({length: src.length / 4}, (_, i) => i).find((i) => src[4 * i] !== 0xffffffff);
    src[4 * k + 1] = list.length; // off + len past the list
    assert.throws(() => addon.verifySameMessageBitsSync(v.ctxs[0], Object.assign({}, one, {src})), new RegExp(`set ${k}:`));
  } finally {
    await v.close();
  }

  const s = new BlsGpuSingleThreadVerifier({device: 0});
  try {
    s.pubkeysSet(0, table, 1);
    s.setIndexList(data.listId, list);
    assert.deepStrictEqual(await s.verifyAggregateSetsSameMessage(mixed[0].sets, mixed[0].message), mixed[0].expected);
    assert.strictEqual(s.metrics.lodestar_bls_aggregated_pubkeys_total, mixed[0].keys);
    assert.deepStrictEqual(await s.verifyAggregateSetsSameMessage(plain.sets, plain.message), plain.expected);
    assert.strictEqual(s.metrics.lodestar_bls_aggregated_pubkeys_total, mixed[0].keys + plain.keys);
  } finally {
    await s.close();
  }
  console.log("same message bits test OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
