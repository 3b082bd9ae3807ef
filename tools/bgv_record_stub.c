/* A recording stand-in for libbgv.so: exactly the bgv_* symbols that
 * lodestar_amd/napi/bgv_addon.c imports, with no device behind them.
 * tools/gen_napi_binding_golden.py builds it as libbgv.so in a temporary
 * directory and links a second copy of the addon against it.
 *
 * Every call appends one line to the file named by BGV_RECORD_LOG: the
 * function, every scalar argument and scalar field of the batch struct, and for
 * every pointer NULL or the SHA-256 of the bytes that the struct's own counts
 * say it addresses.  Outputs are fixed patterns of the index and distinct
 * constants.  A call whose name equals BGV_RECORD_FAIL returns
 * BGV_E_INVALID_ARG with a bgv_last_error text of its own. */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bgv.h"

/* ---------------------------------------------------------------- SHA-256 */
static const uint32_t K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

static void sha_block(uint32_t h[8], const uint8_t* p) {
  uint32_t w[64], a[8];
  for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
  for (int i = 16; i < 64; i++)
    w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
           (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10));
  memcpy(a, h, sizeof a);
  for (int i = 0; i < 64; i++) {
    const uint32_t t1 = a[7] + (ror(a[4], 6) ^ ror(a[4], 11) ^ ror(a[4], 25)) + ((a[4] & a[5]) ^ (~a[4] & a[6])) + K256[i] + w[i];
    const uint32_t t2 = (ror(a[0], 2) ^ ror(a[0], 13) ^ ror(a[0], 22)) + ((a[0] & a[1]) ^ (a[0] & a[2]) ^ (a[1] & a[2]));
    memmove(a + 1, a, 7 * sizeof a[0]);
    a[4] += t1;
    a[0] = t1 + t2;
  }
  for (int i = 0; i < 8; i++) h[i] += a[i];
}

static void sha256_hex(const void* data, size_t len, char out[65]) {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const uint8_t* p = (const uint8_t*)data;
  size_t left = len;
  for (; left >= 64; left -= 64, p += 64) sha_block(h, p);
  uint8_t tail[128] = {0};
  if (left) memcpy(tail, p, left);
  tail[left] = 0x80;
  const size_t tl = left < 56 ? 64 : 128;
  const uint64_t bits = (uint64_t)len * 8;
  for (int i = 0; i < 8; i++) tail[tl - 1 - i] = (uint8_t)(bits >> (8 * i));
  sha_block(h, tail);
  if (tl == 128) sha_block(h, tail + 64);
  for (int i = 0; i < 8; i++) snprintf(out + 8 * i, 9, "%08x", h[i]);
}

/* ---------------------------------------------------------------- the log */
static __thread char g_err[128];
static __thread char g_line[4096];
static __thread size_t g_len;

static void put(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (g_len < sizeof g_line) g_len += (size_t)vsnprintf(g_line + g_len, sizeof g_line - g_len, fmt, ap);
  va_end(ap);
}

static void put_u(const char* name, uint64_t v) { put(" %s=%llu", name, (unsigned long long)v); }
static void put_i(const char* name, int64_t v) { put(" %s=%lld", name, (long long)v); }

/* NULL, or the digest of the `len` bytes at p */
static void put_p(const char* name, const void* p, size_t len) {
  char hex[65];
  if (!p) {
    put(" %s=NULL", name);
    return;
  }
  sha256_hex(p, len, hex);
  put(" %s=%zu:%s", name, len, hex);
}

/* an output pointer: only whether it was given */
static void put_out(const char* name, const void* p) { put(" %s=%s", name, p ? "set" : "NULL"); }

static void begin(const char* fn) {
  g_len = 0;
  put("%s", fn);
}

/* writes the line; the status the call returns */
static int end(const char* fn) {
  const char* path = getenv("BGV_RECORD_LOG");
  const char* fail = getenv("BGV_RECORD_FAIL");
  const int st = fail && !strcmp(fail, fn) ? BGV_E_INVALID_ARG : BGV_OK;
  if (st != BGV_OK) snprintf(g_err, sizeof g_err, "scripted failure of %s", fn);
  put(" -> %d\n", st);
  if (path) {
    FILE* f = fopen(path, "a");
    if (f) {
      fputs(g_line, f);
      fclose(f);
    }
  }
  return st;
}

struct bgv_ctx {
  uint32_t partial_jobs;
};

/* ------------------------------------------------------------ the entries */
int bgv_abi_version(void) { return 4; }
const char* bgv_build_id(void) { return "record-stub"; }
const char* bgv_last_error(void) { return g_err; }

const char* bgv_set_code_name(int code) {
  static const char* name[] = {"BLST_SUCCESS", "BLST_BAD_ENCODING", "BLST_POINT_NOT_ON_CURVE", "BLST_POINT_NOT_IN_GROUP"};
  return code >= 0 && code < 4 ? name[code] : "BLST_STUB_OTHER";
}

void bgv_cfg_default(bgv_cfg* cfg) {
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->split = cfg->miller = cfg->miller_steps = cfg->hash_dedup = -1;
}

int bgv_open_cfg(int device, const bgv_cfg* cfg, bgv_ctx** out) {
  begin("bgv_open_cfg");
  put_i("device", device);
  put_i("cu_split", cfg->cu_split);
  put_i("split", cfg->split);
  put_i("miller", cfg->miller);
  put_i("hash_dedup", cfg->hash_dedup);
  put_i("miller_steps", cfg->miller_steps);
  const int st = end("bgv_open_cfg");
  if (st == BGV_OK) *out = (bgv_ctx*)calloc(1, sizeof **out);
  return st;
}

int bgv_close(bgv_ctx* ctx) {
  begin("bgv_close");
  const int st = end("bgv_close");
  free(ctx);
  return st;
}

int bgv_pubkeys_set(bgv_ctx* ctx, uint32_t first_index, uint32_t n, const uint8_t* data, uint32_t format) {
  (void)ctx;
  begin("bgv_pubkeys_set");
  put_u("first_index", first_index);
  put_u("n", n);
  put_u("format", format);
  put_p("data", data, (size_t)n * (format == BGV_PK_UNCOMPRESSED_96 ? 96 : 48));
  return end("bgv_pubkeys_set");
}

int bgv_pubkeys_count(bgv_ctx* ctx, uint32_t* count) {
  (void)ctx;
  begin("bgv_pubkeys_count");
  *count = 77;
  return end("bgv_pubkeys_count");
}

int bgv_pubkeys_validate(bgv_ctx* ctx, const uint8_t* pk48, uint32_t n, int32_t* codes) {
  (void)ctx;
  begin("bgv_pubkeys_validate");
  put_u("n", n);
  put_p("pk48", pk48, 48 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) codes[i] = (int32_t)(i % 4);
  return end("bgv_pubkeys_validate");
}

static void fill_jobs(int32_t* job_result, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) job_result[i] = i % 4 == 3 ? -(int32_t)(i % 5 + 1) : (int32_t)(i % 3 != 0);
}

static void fill_stats(bgv_stats* s, uint32_t base) {
  memset(s, 0, sizeof *s);
  s->total_ms = 1.5f + (float)base;
  s->batch_retries = base + 7;
  s->batch_sigs_success = base + 11;
  s->pubkeys_aggregated = base + 13;
}

static void put_batch(const bgv_batch* b) {
  put_u("n_sets", b->n_sets);
  put_u("n_jobs", b->n_jobs);
  put_p("job_offsets", b->job_offsets, 4 * ((size_t)b->n_jobs + 1));
  put_p("pk_offsets", b->pk_offsets, 4 * ((size_t)b->n_sets + 1));
  put_p("pk_indices", b->pk_indices, b->pk_offsets ? 4 * (size_t)b->pk_offsets[b->n_sets] : 0);
  put_p("raw_pks", b->raw_pks, 96 * (size_t)b->n_raw);
  put_u("n_raw", b->n_raw);
  put_p("msgs", b->msgs, 32 * (size_t)b->n_sets);
  put_p("sigs", b->sigs, 192 * (size_t)b->n_sets);
  put_p("sig_len", b->sig_len, 4 * (size_t)b->n_sets);
  put_p("scalars", b->scalars, 8 * (size_t)b->n_sets);
  put_u("on_device", b->on_device);
}

int bgv_verify(bgv_ctx* ctx, const bgv_batch* batch, int32_t* job_result, int32_t* set_code, bgv_stats* stats) {
  (void)ctx;
  begin("bgv_verify");
  put_batch(batch);
  put_out("job_result", job_result);
  put_out("set_code", set_code);
  put_out("stats", stats);
  fill_jobs(job_result, batch->n_jobs);
  if (stats) fill_stats(stats, 0);
  return end("bgv_verify");
}

int bgv_last_stats(bgv_ctx* ctx, bgv_stats* stats) {
  (void)ctx;
  begin("bgv_last_stats");
  fill_stats(stats, 100);
  return end("bgv_last_stats");
}

int bgv_partial(bgv_ctx* ctx, const bgv_batch* batch, uint8_t* miller576, int32_t* set_code, int32_t* job_result, int32_t* ok) {
  begin("bgv_partial");
  put_batch(batch);
  put_out("miller576", miller576);
  put_out("set_code", set_code);
  put_out("job_result", job_result);
  ctx->partial_jobs = batch->n_jobs;
  fill_jobs(job_result, batch->n_jobs);
  for (int i = 0; i < 576; i++) miller576[i] = (uint8_t)(3 * i + 1);
  *ok = (int32_t)(batch->n_jobs % 2);
  return end("bgv_partial");
}

int bgv_partial_finish(bgv_ctx* ctx, int32_t* job_result, bgv_stats* stats) {
  begin("bgv_partial_finish");
  put_u("pending_jobs", ctx->partial_jobs);
  fill_jobs(job_result, ctx->partial_jobs);
  fill_stats(stats, 200);
  return end("bgv_partial_finish");
}

int bgv_combine_final(bgv_ctx* ctx, const uint8_t* millers576, uint32_t n, int32_t* is_one) {
  (void)ctx;
  begin("bgv_combine_final");
  put_u("n", n);
  put_p("millers576", millers576, 576 * (size_t)n);
  *is_one = (int32_t)(n % 2);
  return end("bgv_combine_final");
}

int bgv_verify_bits(bgv_ctx* ctx, const bgv_bits_batch* b, int32_t* job_result, int32_t* set_code, bgv_stats* stats) {
  (void)ctx;
  begin("bgv_verify_bits");
  put_u("n_sets", b->n_sets);
  put_u("n_jobs", b->n_jobs);
  put_p("job_offsets", b->job_offsets, 4 * ((size_t)b->n_jobs + 1));
  put_p("src", b->src, 16 * (size_t)b->n_sets);
  put_p("bits", b->bits, b->bits_len);
  put_u("bits_len", b->bits_len);
  put_p("pk_indices", b->pk_indices, 4 * (size_t)b->n_indices);
  put_u("n_indices", b->n_indices);
  put_p("raw_pks", b->raw_pks, 96 * (size_t)b->n_raw);
  put_u("n_raw", b->n_raw);
  put_p("msgs", b->msgs, 32 * (size_t)b->n_sets);
  put_p("sigs", b->sigs, 192 * (size_t)b->n_sets);
  put_p("sig_len", b->sig_len, 4 * (size_t)b->n_sets);
  put_p("scalars", b->scalars, 8 * (size_t)b->n_sets);
  put_u("on_device", b->on_device);
  put_out("job_result", job_result);
  put_out("set_code", set_code);
  put_out("stats", stats);
  fill_jobs(job_result, b->n_jobs);
  if (stats) fill_stats(stats, 300);
  return end("bgv_verify_bits");
}

static void fill_sets(uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats, uint32_t n, uint32_t base) {
  for (uint32_t i = 0; i < n; i++) {
    set_valid[i] = i % 3 != 0;
    set_code[i] = (int32_t)(i % 5);
  }
  if (!stats) return;
  memset(stats, 0, sizeof *stats);
  stats->n_segments = base + 41;
  stats->hashes = base + 42;
  stats->pairs = base + 43;
  stats->groups_retried = base + 44;
  stats->sets_retried = base + 45;
  stats->total_ms = 2.5f + (float)base;
}

static void put_sm_outputs(const uint8_t* set_valid, const int32_t* set_code, const bgv_sm_stats* stats) {
  put_out("set_valid", set_valid);
  put_out("set_code", set_code);
  put_out("stats", stats);
}

static void put_sm_batch(const bgv_sm_batch* b) {
  put_u("n_sets", b->n_sets);
  put_u("n_groups", b->n_groups);
  put_p("group_offsets", b->group_offsets, 4 * ((size_t)b->n_groups + 1));
  put_p("pk_indices", b->pk_indices, 4 * (size_t)b->n_sets);
  put_p("raw_pks", b->raw_pks, 96 * (size_t)b->n_raw);
  put_u("n_raw", b->n_raw);
  put_p("msgs", b->msgs, 32 * (size_t)b->n_groups);
  put_p("sigs", b->sigs, 192 * (size_t)b->n_sets);
  put_p("sig_len", b->sig_len, 4 * (size_t)b->n_sets);
  put_p("scalars", b->scalars, 8 * (size_t)b->n_sets);
  put_u("on_device", b->on_device);
}

int bgv_verify_same_message(bgv_ctx* ctx, const bgv_sm_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  (void)ctx;
  begin("bgv_verify_same_message");
  put_sm_batch(b);
  put_sm_outputs(set_valid, set_code, stats);
  fill_sets(set_valid, set_code, stats, b->n_sets, 0);
  return end("bgv_verify_same_message");
}

int bgv_verify_same_message_aggregate(bgv_ctx* ctx, const bgv_sm_batch* b, const bgv_sm_agg* agg, uint8_t* set_valid,
                                      int32_t* set_code, bgv_sm_stats* stats) {
  (void)ctx;
  begin("bgv_verify_same_message_aggregate");
  put_sm_batch(b);
  put_p("take", agg->take, b->n_sets);
  put_p("prev_sig96", agg->prev_sig96, 96 * (size_t)b->n_groups);
  put_out("agg_sig96", agg->agg_sig96);
  put_out("agg_count", agg->agg_count);
  put_out("agg_code", agg->agg_code);
  put_sm_outputs(set_valid, set_code, stats);
  fill_sets(set_valid, set_code, stats, b->n_sets, 10);
  for (uint32_t g = 0; b->n_sets && g < b->n_groups; g++) {
    for (int k = 0; k < 96; k++) agg->agg_sig96[96 * (size_t)g + k] = (uint8_t)(7 * g + k);
    if (agg->agg_count) agg->agg_count[g] = g + 1;
    if (agg->agg_code) agg->agg_code[g] = g % 2 ? 2 : 0;
  }
  return end("bgv_verify_same_message_aggregate");
}

int bgv_verify_same_message_agg(bgv_ctx* ctx, const bgv_sma_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  (void)ctx;
  begin("bgv_verify_same_message_agg");
  put_u("n_sets", b->n_sets);
  put_u("n_groups", b->n_groups);
  put_p("group_offsets", b->group_offsets, 4 * ((size_t)b->n_groups + 1));
  put_p("pk_offsets", b->pk_offsets, 4 * ((size_t)b->n_sets + 1));
  put_p("pk_indices", b->pk_indices, b->pk_offsets ? 4 * (size_t)b->pk_offsets[b->n_sets] : 0);
  put_p("raw_pks", b->raw_pks, 96 * (size_t)b->n_raw);
  put_u("n_raw", b->n_raw);
  put_p("msgs", b->msgs, 32 * (size_t)b->n_groups);
  put_p("sigs", b->sigs, 192 * (size_t)b->n_sets);
  put_p("sig_len", b->sig_len, 4 * (size_t)b->n_sets);
  put_p("scalars", b->scalars, 8 * (size_t)b->n_sets);
  put_u("on_device", b->on_device);
  put_sm_outputs(set_valid, set_code, stats);
  fill_sets(set_valid, set_code, stats, b->n_sets, 20);
  return end("bgv_verify_same_message_agg");
}

int bgv_verify_same_message_bits(bgv_ctx* ctx, const bgv_smb_batch* b, uint8_t* set_valid, int32_t* set_code, bgv_sm_stats* stats) {
  (void)ctx;
  begin("bgv_verify_same_message_bits");
  put_u("n_sets", b->n_sets);
  put_u("n_groups", b->n_groups);
  put_p("group_offsets", b->group_offsets, 4 * ((size_t)b->n_groups + 1));
  put_p("src", b->src, 16 * (size_t)b->n_sets);
  put_p("bits", b->bits, b->bits_len);
  put_u("bits_len", b->bits_len);
  put_p("pk_indices", b->pk_indices, 4 * (size_t)b->n_indices);
  put_u("n_indices", b->n_indices);
  put_p("raw_pks", b->raw_pks, 96 * (size_t)b->n_raw);
  put_u("n_raw", b->n_raw);
  put_p("msgs", b->msgs, 32 * (size_t)b->n_groups);
  put_p("sigs", b->sigs, 192 * (size_t)b->n_sets);
  put_p("sig_len", b->sig_len, 4 * (size_t)b->n_sets);
  put_p("scalars", b->scalars, 8 * (size_t)b->n_sets);
  put_u("on_device", b->on_device);
  put_sm_outputs(set_valid, set_code, stats);
  fill_sets(set_valid, set_code, stats, b->n_sets, 30);
  return end("bgv_verify_same_message_bits");
}

int bgv_index_list_set(bgv_ctx* ctx, uint32_t list_id, const uint32_t* indices, uint32_t n) {
  (void)ctx;
  begin("bgv_index_list_set");
  put_u("list_id", list_id);
  put_u("n", n);
  put_p("indices", indices, 4 * (size_t)n);
  return end("bgv_index_list_set");
}

int bgv_index_list_len(bgv_ctx* ctx, uint32_t list_id, uint32_t* n) {
  (void)ctx;
  begin("bgv_index_list_len");
  put_u("list_id", list_id);
  *n = 10 * list_id + 5;
  return end("bgv_index_list_len");
}

int bgv_index_list_sums(bgv_ctx* ctx, uint32_t list_id, uint32_t enable) {
  (void)ctx;
  begin("bgv_index_list_sums");
  put_u("list_id", list_id);
  put_u("enable", enable);
  return end("bgv_index_list_sums");
}

int bgv_index_list_has_sums(bgv_ctx* ctx, uint32_t list_id, uint32_t* has) {
  (void)ctx;
  begin("bgv_index_list_has_sums");
  put_u("list_id", list_id);
  *has = list_id & 1;
  return end("bgv_index_list_has_sums");
}

int bgv_bits_path_stats(bgv_ctx* ctx, bgv_bits_path* out) {
  (void)ctx;
  begin("bgv_bits_path_stats");
  out->sets_complement = 61;
  out->keys_expanded = 62;
  out->keys_gathered = 63;
  return end("bgv_bits_path_stats");
}

int bgv_hash_stats(bgv_ctx* ctx, bgv_hash_path* out) {
  (void)ctx;
  begin("bgv_hash_stats");
  out->sets = 21;
  out->hashes = 22;
  out->dedup = 23;
  return end("bgv_hash_stats");
}

int bgv_pair_merge(bgv_ctx* ctx, int32_t mode) {
  (void)ctx;
  begin("bgv_pair_merge");
  put_i("mode", mode);
  return end("bgv_pair_merge");
}

int bgv_pair_stats(bgv_ctx* ctx, bgv_pair_path* out) {
  (void)ctx;
  begin("bgv_pair_stats");
  out->sets = 31;
  out->pairs = 32;
  out->merged = 33;
  out->fallback = 34;
  return end("bgv_pair_stats");
}

int bgv_sm_retry(bgv_ctx* ctx, int32_t mode) {
  (void)ctx;
  begin("bgv_sm_retry");
  put_i("mode", mode);
  return end("bgv_sm_retry");
}

int bgv_sm_retry_stats(bgv_ctx* ctx, bgv_sm_retry_path* out) {
  (void)ctx;
  begin("bgv_sm_retry_stats");
  out->mode = 51;
  out->segments = 52;
  out->subs = 53;
  out->subs_failed = 54;
  out->leaves = 55;
  out->pairs = 56;
  out->hashes = 57;
  return end("bgv_sm_retry_stats");
}
