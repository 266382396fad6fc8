/* model_exercise -- the host layer on the model HIP runtime from a program of its own (no Python), for a sanitizer build:
 *
 *   python -c "from nanorq_amd import build; build.build_model_exercise(sanitize=True)" && tests/emu/model_exercise_asan
 *
 * builds tests/emu/libnanorq_model_asan.so -- every host source of the library and the model with
 * -fsanitize=address,undefined -- and this program against it, and runs the pool scenarios and the object layer's `fail_after`
 * sweeps of tests/test_host_model.py (groups b and e) once: the error paths of nrq_device.hip's host code and of nanorq_api.c
 * under AddressSanitizer / UBSan, without a GPU.  Kernels do not run (hip_model.h); packets are made without an encoder: source
 * symbols are slices of the object, a repair symbol's bytes do not matter to the host layer.
 * Exit status 0 = no hazard, every convention held, every sweep reached its runtime calls (and no sanitizer report). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hip_model.h"
#include "io.h"
#include "nanorq.h"
#include "nanorq_batch.h"
#include "nanorq_hip.h"

/* (the object layer keeps its contexts for the life of the process: no leak check; identical string literals of one source file
 * that the linker merged are no ODR violation) */
extern "C" const char *__asan_default_options(void) { return "detect_leaks=0:detect_odr_violation=0:halt_on_error=1"; }
extern "C" const char *__ubsan_default_options(void) { return "print_stacktrace=1:halt_on_error=1"; }

static int g_bad = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      if (g_bad++ < 30) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    }                                                            \
  } while (0)

static uint32_t rnd(uint64_t *s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static void no_hazards(const char *where) {
  if (hm_hazard_count() == 0) return;
  std::vector<char> buf(hm_hazards_json(nullptr, 0) + 1);
  hm_hazards_json(buf.data(), buf.size());
  CHECK(false, "%s: hazards %.1500s", where, buf.data());
  hm_hazards_clear();
}

/* ---- b. the pool ---- */
static void books(nrq_ctx *c, size_t b[3]) { CHECK(nrq_dev_pool_books(c, b) == 0, "books"); }
static void pool(void) {
  nrq_ctx *c = nullptr;
  CHECK(nrq_ctx_create(0, nullptr, &c) == 0 && c, "context");
  if (!c) return;
  size_t b[3];
  void *a = nullptr, *p = nullptr, *q = nullptr;
  CHECK(nrq_dev_alloc(c, 1 << 20, &a) == 0 && nrq_dev_free(c, a) == 0, "alloc / free");
  CHECK(nrq_dev_alloc(c, (1 << 20) - 4096, &p) == 0 && p == a, "a request within the rule takes the cached block");
  CHECK(nrq_dev_free(c, p) == 0, "free");
  CHECK(nrq_dev_alloc(c, 1, &p) == 0 && p != a, "a small request leaves the big block alone");
  CHECK(nrq_dev_free(c, p) == 0 && nrq_dev_free(c, p) == -1, "a second free is refused");
  books(c, b);
  CHECK(b[0] == 2 && b[1] == 2, "two blocks, both cached once: %zu %zu", b[0], b[1]);
  CHECK(nrq_dev_free(c, (uint8_t *)a + 4096) == -1, "an inner address is refused");
  CHECK(nrq_dev_trim(c) == 0, "trim");
  books(c, b);
  CHECK(b[0] == 0 && b[1] == 0 && b[2] == 0, "nothing left after the trim");
  for (long long n = 1; n <= 2; n++) { /* the call's first runtime call, then the allocation itself */
    CHECK(nrq_ctx_set_option(c, "fail_after", n) == 0, "fail_after");
    CHECK(nrq_dev_alloc(c, 123456, &q) == -10 && q == nullptr, "an injected failure of the allocation (n = %lld)", n);
    nrq_ctx_set_option(c, "fail_after", 0);
    books(c, b);
    CHECK(b[0] == 0 && b[1] == 0, "the books after a failed allocation");
  }
  uint64_t st = 5;
  std::vector<void *> live;
  for (int step = 0; step < 400; step++) {
    if (!live.empty() && rnd(&st) % 100u < 45u) {
      const size_t k = rnd(&st) % live.size();
      CHECK(nrq_dev_free(c, live[k]) == 0, "free");
      live[k] = live.back();
      live.pop_back();
    } else {
      void *x = nullptr;
      const size_t n = 1 + rnd(&st) % 300000u;
      CHECK(nrq_dev_alloc(c, n, &x) == 0 && x, "alloc");
      uint64_t base = 0, size = 0;
      CHECK(hm_block_of(x, &base, &size, nullptr) && base == (uint64_t)(uintptr_t)x && size >= n, "a block of at least the size asked for");
      for (void *y : live) CHECK(y != x, "one block, two owners");
      CHECK(nrq_dev_memset(c, x, 0x5A, n) == 0, "memset");
      live.push_back(x);
    }
    if (step % 97 == 0) CHECK(nrq_dev_trim(c) == 0, "trim");
  }
  CHECK(nrq_ctx_sync(c) == 0, "sync");
  nrq_ctx_destroy(c); /* (with blocks outstanding) */
  no_hazards("pool");
}

/* ---- e. the object layer under fault injection ---- */
struct Packets {
  size_t F = 0, T = 0, K = 0;
  std::vector<uint8_t> data;
  std::vector<uint32_t> tags;
  std::vector<size_t> off; /* of a source symbol in the object, (size_t)-1 for a repair symbol */
  uint64_t oc = 0;
  uint32_t os = 0;
  size_t Z = 0;
};
static Packets make_packets(size_t F, size_t T, size_t K, unsigned loss_pct, unsigned oh, uint64_t seed) {
  Packets p;
  p.F = F; p.T = T; p.K = K;
  p.data.resize(F);
  uint64_t st = seed;
  for (size_t i = 0; i < F; i++) p.data[i] = (uint8_t)rnd(&st);
  nanorq *enc = nanorq_encoder_new_ex(F, (uint16_t)T, (uint16_t)K, 0, 8);
  if (!enc) { CHECK(false, "encoder"); return p; }
  p.Z = nanorq_blocks(enc);
  size_t off = 0;
  for (size_t sbn = 0; sbn < p.Z; sbn++) {
    const size_t k = nanorq_block_symbols(enc, (uint8_t)sbn);
    uint32_t dropped = 0;
    for (uint32_t esi = 0; esi < k; esi++) {
      if (rnd(&st) % 100u < loss_pct) { dropped++; continue; }
      p.tags.push_back(nanorq_tag((uint8_t)sbn, esi));
      p.off.push_back(off + (size_t)esi * T);
    }
    for (uint32_t esi = (uint32_t)k; esi < k + dropped + oh; esi++) {
      p.tags.push_back(nanorq_tag((uint8_t)sbn, esi));
      p.off.push_back((size_t)-1);
    }
    off += k * T;
  }
  p.oc = nanorq_oti_common(enc);
  p.os = nanorq_oti_scheme_specific(enc);
  nanorq_free(enc);
  return p;
}
/* packets [first, first + n) of p in a page-locked buffer */
static uint8_t *blob_of(const Packets &p, const std::vector<uint32_t> &idx) {
  uint8_t *pk = (uint8_t *)nanorq_pinned_alloc(idx.size() * p.T + 1);
  if (!pk) return nullptr;
  for (size_t i = 0; i < idx.size(); i++) {
    uint8_t *d = pk + i * p.T;
    const size_t o = p.off[idx[i]];
    memset(d, 0xA7, p.T);
    if (o != (size_t)-1) {
      const size_t n = o + p.T <= p.F ? p.T : p.F - o;
      memset(d, 0, p.T);
      memcpy(d, p.data.data() + o, n);
    }
  }
  return pk;
}
static void received_right(const Packets &p, const uint8_t *out, const char *where, long long n) {
  size_t bad = 0;
  for (size_t i = 0; i < p.off.size(); i++) {
    const size_t o = p.off[i];
    if (o == (size_t)-1) continue;
    const size_t m = o + p.T <= p.F ? p.T : p.F - o;
    bad += memcmp(out + o, p.data.data() + o, m) != 0;
  }
  CHECK(bad == 0, "%s n=%lld: %zu received source symbols are not in the output", where, n, bad);
}
static int faults_now(void) { return nanorq_hip_option(0, "faults_injected", 0); }

static void batch(bool async) {
  const Packets p = make_packets(5 * 120 * 256 - 9, 256, 120, 10, 3, 5);
  std::vector<uint32_t> all(p.tags.size());
  for (size_t i = 0; i < all.size(); i++) all[i] = (uint32_t)i;
  int hit = 0, rolled = 0;
  for (long long n = 1; n <= 96; n += (n < 40 ? 1 : 8)) {
    nanorq *dq = nanorq_decoder_new(p.oc, p.os);
    struct ioctx *oio = ioctx_from_pinned_mem(p.F);
    if (!dq || !oio) { CHECK(false, "decoder"); return; }
    uint8_t *out = (uint8_t *)ioctx_mem_base(oio);
    memset(out, 0, p.F);
    uint8_t *pk = blob_of(p, all);
    std::vector<int> res(all.size(), 77);
    const int before = faults_now();
    nanorq_hip_option(0, "fail_after", n);
    const size_t added = (async ? nanorq_decoder_add_symbols_async : nanorq_decoder_add_symbols)(dq, pk, p.tags.data(), (uint32_t)all.size(), res.data(), oio);
    nanorq_hip_option(0, "fail_after", 0);
    hit += faults_now() > before;
    size_t ok = 0;
    std::vector<uint32_t> again;
    for (size_t i = 0; i < res.size(); i++) {
      CHECK(res[i] == NANORQ_SYM_ADDED || res[i] == NANORQ_SYM_ERR, "batch n=%lld: result %d", n, res[i]);
      ok += res[i] == NANORQ_SYM_ADDED;
      if (res[i] == NANORQ_SYM_ERR) again.push_back((uint32_t)i);
    }
    CHECK(added == ok, "batch n=%lld: %zu reported, %zu in the results", n, added, ok);
    uint8_t *pk2 = nullptr;
    if (!again.empty()) {
      rolled += added == 0;
      pk2 = blob_of(p, again);
      std::vector<uint32_t> t2;
      for (uint32_t i : again) t2.push_back(p.tags[i]);
      if (n % 2) {
        std::vector<int> r2(again.size(), 77);
        CHECK((async ? nanorq_decoder_add_symbols_async : nanorq_decoder_add_symbols)(dq, pk2, t2.data(), (uint32_t)t2.size(), r2.data(), oio) == t2.size(),
              "batch n=%lld: the retry", n);
      } else {
        for (size_t i = 0; i < t2.size(); i++) CHECK(nanorq_decoder_add_symbol(dq, pk2 + i * p.T, t2[i], oio) == NANORQ_SYM_ADDED, "batch n=%lld: retry per symbol", n);
      }
    }
    CHECK(nanorq_repair_all(dq, oio) == p.Z, "batch n=%lld: repair_all", n);
    received_right(p, out, "batch", n);
    nanorq_free(dq);
    nanorq_pinned_free(pk);
    if (pk2) nanorq_pinned_free(pk2);
    oio->destroy(oio);
    no_hazards(async ? "batch (async)" : "batch");
  }
  CHECK(hit >= 20 && rolled >= 3, "the batch sweep did not reach the runtime calls: hit %d, taken back %d", hit, rolled);
}

static void repair_all(bool device) {
  const Packets p = make_packets(6 * 300 * 512, 512, 300, 8, 2, 9);
  std::vector<uint32_t> all(p.tags.size());
  for (size_t i = 0; i < all.size(); i++) all[i] = (uint32_t)i;
  int hit = 0;
  for (long long n = 1; n <= 200; n += (n < 60 ? 2 : 40)) {
    nanorq *dq = nanorq_decoder_new(p.oc, p.os);
    struct ioctx *oio = ioctx_from_pinned_mem(p.F);
    if (!dq || !oio) { CHECK(false, "decoder"); return; }
    uint8_t *out = (uint8_t *)ioctx_mem_base(oio);
    memset(out, 0, p.F);
    uint8_t *pk = blob_of(p, all);
    if (device) {
      CHECK(nanorq_decoder_add_symbols(dq, pk, p.tags.data(), (uint32_t)all.size(), nullptr, oio) == all.size(), "repair_all: feed");
    } else {
      for (size_t i = 0; i < all.size(); i++) CHECK(nanorq_decoder_add_symbol(dq, pk + i * p.T, p.tags[i], oio) == NANORQ_SYM_ADDED, "repair_all: feed");
    }
    const int before = faults_now();
    nanorq_hip_option(0, "fail_after", n);
    const size_t done = nanorq_repair_all(dq, oio);
    nanorq_hip_option(0, "fail_after", 0);
    hit += faults_now() > before;
    CHECK(done <= p.Z, "repair_all n=%lld: %zu blocks", n, done);
    CHECK(nanorq_repair_all(dq, oio) == p.Z, "repair_all n=%lld: the second call", n);
    received_right(p, out, "repair_all", n);
    nanorq_free(dq);
    nanorq_pinned_free(pk);
    oio->destroy(oio);
    no_hazards(device ? "repair_all (device-resident)" : "repair_all (host-resident)");
  }
  CHECK(hit >= 10, "the repair_all sweep did not reach the runtime calls: hit %d", hit);
}

static void per_block(void) {
  const Packets p = make_packets(3 * 200 * 128, 128, 200, 10, 2, 31);
  std::vector<uint32_t> all(p.tags.size());
  for (size_t i = 0; i < all.size(); i++) all[i] = (uint32_t)i;
  int hit = 0;
  std::vector<uint8_t> in(p.data), buf(p.T);
  for (long long n = 1; n < 30; n++) {
    nanorq *rq = nanorq_encoder_new_ex(p.F, (uint16_t)p.T, (uint16_t)p.K, 0, 8);
    struct ioctx *io = ioctx_from_mem(in.data(), p.F);
    int before = faults_now();
    nanorq_hip_option(0, "fail_after", n);
    const bool ok = nanorq_generate_symbols(rq, 1, io);
    const size_t got = ok ? nanorq_encode(rq, buf.data(), (uint32_t)p.K + 1, 1, io) : 0;
    nanorq_hip_option(0, "fail_after", 0);
    hit += faults_now() > before;
    CHECK(got == 0 || got == p.T, "per block n=%lld: nanorq_encode gave %zu", n, got);
    if (!ok || got != p.T) CHECK(nanorq_encode(rq, buf.data(), (uint32_t)p.K + 1, 1, io) == p.T, "per block n=%lld: the retry of nanorq_encode", n);
    nanorq_free(rq);
    io->destroy(io);
    nanorq *dq = nanorq_decoder_new(p.oc, p.os);
    std::vector<uint8_t> out(p.F, 0);
    struct ioctx *oio = ioctx_from_mem(out.data(), p.F);
    uint8_t *pk = blob_of(p, all);
    for (size_t i = 0; i < all.size(); i++) nanorq_decoder_add_symbol(dq, pk + i * p.T, p.tags[i], oio);
    before = faults_now();
    nanorq_hip_option(0, "fail_after", n);
    const bool ok0 = nanorq_repair_block(dq, oio, 0);
    nanorq_hip_option(0, "fail_after", 0);
    hit += faults_now() > before;
    if (!ok0) CHECK(nanorq_num_missing(dq, 0) > 0, "per block n=%lld: a failed repair_block left no gaps", n);
    for (uint8_t b = 0; b < 3; b++) CHECK(nanorq_repair_block(dq, oio, b), "per block n=%lld: the retry of block %u", n, b);
    received_right(p, out.data(), "per block", n);
    nanorq_free(dq);
    nanorq_pinned_free(pk);
    oio->destroy(oio);
    no_hazards("per block");
  }
  CHECK(hit >= 10, "the per-block sweep did not reach the runtime calls: hit %d", hit);
}

int main(void) {
  setenv("NANORQ_HIP_FAULT_INJECT", "1", 1);
  setenv("NRQ_HOST_PLANNER", "1", 1);
  pool();
  batch(false);
  batch(true);
  repair_all(true);
  repair_all(false);
  per_block();
  uint64_t c[8];
  hm_counters(c);
  printf("model_exercise: %llu operations, %llu launches, %d failures\n", (unsigned long long)c[0], (unsigned long long)c[1], g_bad);
  return g_bad ? 1 : 0;
}
