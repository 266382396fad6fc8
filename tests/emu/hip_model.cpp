/* The model HIP runtime (hip_model.h says what it models and what it assumes).  It defines the runtime functions the host layer
 * calls, with the runtime's own prototypes, over a table of allocations and a vector clock per stream.  Built by g++ / hipcc as
 * plain C++ into tests/emu/libnanorq_model.so next to the host layer; never linked into the product library. */
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "hip_model.h"

namespace {

typedef std::vector<uint64_t> VC; /* vector clock: entry i = operations of stream i known to be over (0 = the host has none) */

void vc_join(VC &a, const VC &b) {
  if (a.size() < b.size()) a.resize(b.size(), 0);
  for (size_t i = 0; i < b.size(); i++) a[i] = std::max(a[i], b[i]);
}
uint64_t vc_at(const VC &a, size_t i) { return i < a.size() ? a[i] : 0; }

struct StreamM {
  int idx = 0;
  bool live = true;
  VC clock; /* clock[idx] = number of the stream's last operation */
};
struct EventM {
  bool recorded = false, live = true;
  VC vc;
};

struct OpInfo {
  std::string what; /* "hipMemcpyAsync H2D 4096 B", "launch nrq_gen_kernel", ... */
  const void *site; /* return address of the runtime call, or null */
  std::string where; /* file:line of a launch */
  int sidx;
  uint64_t epoch;
};

struct Access {
  uint32_t op;
  int sidx;
  uint64_t epoch;
  size_t off, len;
  bool write;
};

enum { K_DEV = 0, K_PIN = 1, K_REG = 2 };
struct Alloc {
  uintptr_t base = 0;
  size_t size = 0;
  int kind = K_DEV;
  bool live = true;
  uint32_t serial = 0;
  const void *site = nullptr;
  /* Device memory holds an address only if a copy brought one (kernels do not run): launches look for addresses only in device
   * allocations a copy has carried a word of the model's ranges into.  Page-locked memory is written by the host unseen: always. */
  bool may_hold_addresses = false;
  std::vector<Access> acc;
};

/* a deferred device -> page-locked copy, or the watch over the source of a page-locked -> device copy (H4) */
struct Pending {
  uint32_t op;
  int sidx;
  uint64_t epoch;
  bool download;
  uintptr_t host; /* page-locked side */
  size_t len;
  Alloc *halloc;
  uint32_t hserial;
  std::vector<uint8_t> bytes; /* download: the source as it was at enqueue */
  uint64_t hash = 0;          /* upload: of the source at enqueue */
};

struct Hazard {
  std::string kind, detail;
  uint32_t op_a, op_b; /* op_b = the later one (the one that found it); op_a may be ~0u */
  uintptr_t base;
  size_t size;
  int akind;
};

struct Model {
  std::mutex mu;
  uint8_t *dev_lo = nullptr, *pin_lo = nullptr;
  size_t dev_cap = 0, pin_cap = 0, dev_used = 0, pin_used = 0;
  std::map<uintptr_t, std::unique_ptr<Alloc>> live; /* by base */
  std::vector<std::unique_ptr<Alloc>> dead;
  uint32_t serial = 0;
  std::vector<std::unique_ptr<StreamM>> streams; /* [0] = the null stream */
  std::vector<std::unique_ptr<EventM>> events;
  VC host;
  std::vector<OpInfo> ops;
  std::vector<Pending> pending;
  std::vector<Hazard> hazards;
  std::map<const void *, std::string> kernels;
  struct Effect { std::string name; hm_effect_fn fn; bool exact; };
  std::vector<Effect> effects;
  StreamM *cur_s = nullptr; /* the launch whose effect is running */
  uint32_t cur_op = 0;
  unsigned cur_grid[3] = {1, 1, 1};
  uint64_t n_launch = 0, n_copy = 0, n_unrec = 0, n_stale = 0, n_unnamed = 0;

  Model() {
    streams.emplace_back(new StreamM());
    streams[0]->clock.assign(1, 0);
    for (size_t cap = (size_t)256 << 30; cap >= ((size_t)4 << 30) && !dev_lo; cap >>= 1) {
      void *p = mmap(nullptr, cap + cap / 4, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
      if (p == MAP_FAILED) continue;
      dev_lo = (uint8_t *)p;
      dev_cap = cap;
      pin_lo = dev_lo + cap;
      pin_cap = cap / 4;
    }
  }
};
Model &M() {
  static Model *m = new Model(); /* (never destroyed: contexts may be torn down by static destructors after ours) */
  return *m;
}

bool in_dev(const Model &m, uintptr_t p) { return p >= (uintptr_t)m.dev_lo && p < (uintptr_t)m.dev_lo + m.dev_cap; }
bool in_pin(const Model &m, uintptr_t p) { return p >= (uintptr_t)m.pin_lo && p < (uintptr_t)m.pin_lo + m.pin_cap; }

Alloc *find(Model &m, uintptr_t p) {
  auto it = m.live.upper_bound(p);
  if (it == m.live.begin()) return nullptr;
  --it;
  Alloc *a = it->second.get();
  return p < a->base + a->size ? a : nullptr;
}
const Alloc *find_dead(const Model &m, uintptr_t p) {
  for (auto it = m.dead.rbegin(); it != m.dead.rend(); ++it)
    if (p >= (*it)->base && p < (*it)->base + (*it)->size) return it->get();
  return nullptr;
}

std::string site_name(const void *ra) {
  if (!ra) return "";
  Dl_info di;
  char buf[256];
  if (dladdr(ra, &di) && di.dli_sname) snprintf(buf, sizeof(buf), "%s+0x%zx", di.dli_sname, (size_t)((const char *)ra - (const char *)di.dli_saddr));
  else if (dladdr(ra, &di) && di.dli_fname) snprintf(buf, sizeof(buf), "%s@0x%zx", strrchr(di.dli_fname, '/') ? strrchr(di.dli_fname, '/') + 1 : di.dli_fname, (size_t)((const char *)ra - (const char *)di.dli_fbase));
  else snprintf(buf, sizeof(buf), "%p", ra);
  return buf;
}

StreamM *stream_of(Model &m, hipStream_t h) {
  if (!h) return m.streams[0].get();
  for (auto &s : m.streams)
    if ((void *)s.get() == (void *)h) return s.get();
  return nullptr;
}
EventM *event_of(Model &m, hipEvent_t h) {
  for (auto &e : m.events)
    if ((void *)e.get() == (void *)h) return e.get();
  return nullptr;
}

void hazard(Model &m, const char *kind, uint32_t op_a, uint32_t op_b, const Alloc *a, const std::string &detail) {
  if (m.hazards.size() >= 4096) return;
  Hazard h;
  h.kind = kind; h.detail = detail; h.op_a = op_a; h.op_b = op_b;
  h.base = a ? a->base : 0; h.size = a ? a->size : 0; h.akind = a ? a->kind : -1;
  m.hazards.push_back(h);
}

/* a new operation on `s`: enqueued after everything the host has synchronised with, behind the stream's earlier operations */
uint32_t new_op(Model &m, StreamM *s, const std::string &what, const void *site, const std::string &where = "") {
  vc_join(s->clock, m.host);
  if (s->clock.size() <= (size_t)s->idx) s->clock.resize(s->idx + 1, 0);
  s->clock[s->idx]++;
  OpInfo o;
  o.what = what; o.site = site; o.where = where; o.sidx = s->idx; o.epoch = s->clock[s->idx];
  m.ops.push_back(o);
  return (uint32_t)(m.ops.size() - 1);
}

bool done_for_host(const Model &m, int sidx, uint64_t epoch) { return vc_at(m.host, sidx) >= epoch; }

/* operation `op` (of stream s, clock already advanced) touches [off, off + len) of a */
void touch(Model &m, Alloc *a, StreamM *s, uint32_t op, size_t off, size_t len, bool write, const char *note = "") {
  if (!len) return;
  std::vector<Access> keep;
  keep.reserve(a->acc.size() + 1);
  for (const Access &x : a->acc) {
    const bool before = vc_at(s->clock, x.sidx) >= x.epoch; /* x happens before op */
    const bool overlap = x.off < off + len && off < x.off + x.len;
    if (!before && overlap && (x.write || write)) {
      char d[320];
      snprintf(d, sizeof(d), "%s/%s, bytes [%zu, %zu) and [%zu, %zu)%s%s", x.write ? "write" : "read", write ? "write" : "read", x.off,
               x.off + x.len, off, off + len, *note ? "; the second reaches it through " : "", note);
      hazard(m, "H1", x.op, op, a, d);
    }
    if (done_for_host(m, x.sidx, x.epoch)) continue;                                          /* every later operation is behind it */
    if (before && x.off >= off && x.off + x.len <= off + len && (write || !x.write)) continue; /* whoever races x races op */
    keep.push_back(x);
  }
  Access n;
  n.op = op; n.sidx = s->idx; n.epoch = s->clock[s->idx]; n.off = off; n.len = len; n.write = write;
  keep.push_back(n);
  a->acc.swap(keep);
}

int pending_on(const Model &m, const Alloc *a) {
  int n = 0;
  for (const Access &x : a->acc)
    if (!done_for_host(m, x.sidx, x.epoch)) n++;
  return n;
}

uint64_t hash_bytes(const uint8_t *p, size_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, p + i, 8);
    h = (h ^ w) * 0x100000001B3ull;
    h ^= h >> 29;
  }
  for (; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
  return h;
}

/* the model itself has written [lo, lo + n) of page-locked memory (the poison of a deferred download, or its arrival): whether
 * that write is ordered against a pending upload out of the same bytes is H1's question and was answered when the download was
 * enqueued; the watch over the upload's source follows the bytes, so that H4 stays about what the HOST wrote */
void rewatch(Model &m, uintptr_t lo, size_t n) {
  for (Pending &p : m.pending)
    if (!p.download && p.host < lo + n && lo < p.host + p.len) p.hash = hash_bytes((const uint8_t *)p.host, p.len);
}

/* the host has synchronised with something: deferred copies behind it arrive, watched upload sources are compared */
void host_advanced(Model &m) {
  size_t w = 0;
  for (size_t i = 0; i < m.pending.size(); i++) {
    Pending &p = m.pending[i];
    if (!done_for_host(m, p.sidx, p.epoch)) {
      if (w != i) m.pending[w] = std::move(p);
      w++;
      continue;
    }
    Alloc *a = find(m, p.host);
    const bool same = a && a == p.halloc && a->serial == p.hserial && p.host + p.len <= a->base + a->size;
    if (!same) continue; /* released in between: H3 was reported at the release; nothing is touched */
    if (p.download) {
      memcpy((void *)p.host, p.bytes.data(), p.len);
      rewatch(m, p.host, p.len);
    } else if (hash_bytes((const uint8_t *)p.host, p.len) != p.hash)
      hazard(m, "H4", ~0u, p.op, a, "the page-locked source changed between the enqueue of the copy and the host's synchronisation behind it");
  }
  m.pending.resize(w);
}

void sync_stream(Model &m, StreamM *s) {
  vc_join(m.host, s->clock);
  host_advanced(m);
}
void sync_device(Model &m) {
  for (auto &s : m.streams) vc_join(m.host, s->clock);
  host_advanced(m);
}

void *carve(Model &m, bool pin, size_t bytes) {
  const size_t need = ((bytes + 4095) & ~(size_t)4095) + 4096; /* (a page nobody owns behind every allocation) */
  uint8_t *lo = pin ? m.pin_lo : m.dev_lo;
  size_t &used = pin ? m.pin_used : m.dev_used;
  const size_t cap = pin ? m.pin_cap : m.dev_cap;
  if (!lo || used + need > cap) return nullptr;
  void *p = lo + used;
  used += need;
  return p;
}

Alloc *add_alloc(Model &m, uintptr_t base, size_t size, int kind, const void *site) {
  std::unique_ptr<Alloc> a(new Alloc());
  a->base = base; a->size = size; a->kind = kind; a->serial = ++m.serial; a->site = site;
  a->may_hold_addresses = kind != K_DEV;
  Alloc *r = a.get();
  m.live[base] = std::move(a);
  return r;
}
void retire(Model &m, Alloc *a) {
  auto it = m.live.find(a->base);
  a->live = false;
  a->acc.clear();
  if (a->kind != K_REG) madvise((void *)a->base, (a->size + 4095) & ~(size_t)4095, MADV_DONTNEED); /* (the pages go, the addresses stay ours) */
  m.dead.push_back(std::move(it->second));
  m.live.erase(it);
  if (m.dead.size() > 65536) m.dead.erase(m.dead.begin(), m.dead.begin() + 32768);
}

/* a range an operation names: the live allocation that holds all of it, or H2 (and null) */
Alloc *range(Model &m, uint32_t op, const void *p, size_t n, const char *role) {
  const uintptr_t u = (uintptr_t)p;
  Alloc *a = find(m, u);
  char d[200];
  if (a && u + n <= a->base + a->size) return a;
  if (a) {
    snprintf(d, sizeof(d), "%s [%zu, %zu) leaves its allocation of %zu bytes", role, (size_t)(u - a->base), (size_t)(u - a->base) + n, a->size);
    hazard(m, "H2", ~0u, op, a, d);
    return nullptr;
  }
  const Alloc *z = find_dead(m, u);
  if (z) snprintf(d, sizeof(d), "%s %p (+%zu bytes) is in an allocation that was released", role, p, n);
  else snprintf(d, sizeof(d), "%s %p (+%zu bytes) is in no allocation", role, p, n);
  hazard(m, "H2", ~0u, op, z, d);
  return nullptr;
}

const char *err_name(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorNotReady: return "device not ready";
    case hipErrorInvalidResourceHandle: return "invalid resource handle";
    default: return "model runtime error";
  }
}

/* bytes that were just written into `a`: do they carry a word of the model's address ranges? */
void note_written(Model &m, Alloc *a, const void *p, size_t n) {
  if (!a || a->may_hold_addresses) return;
  const uint8_t *q = (const uint8_t *)p;
  size_t i = (8 - ((uintptr_t)q & 7)) & 7; /* (addresses are stored aligned) */
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, q + i, 8);
    if (in_dev(m, (uintptr_t)w) || in_pin(m, (uintptr_t)w)) { a->may_hold_addresses = true; return; }
  }
}

hipError_t do_copy(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t st, bool blocking, const void *site) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  StreamM *s = stream_of(m, st);
  if (!s || !s->live) return hipErrorInvalidResourceHandle;
  if (!n) return hipSuccess;
  if (!dst || !src) return hipErrorInvalidValue;
  m.n_copy++;
  const uintptr_t ud = (uintptr_t)dst, us = (uintptr_t)src;
  Alloc *ad = find(m, ud), *as = find(m, us);
  /* which sides the model owns: a device address, or page-locked host memory; anything else is pageable host memory */
  const bool d_dev = in_dev(m, ud) || kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
  const bool s_dev = in_dev(m, us) || kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
  const bool d_own = d_dev || ad || in_pin(m, ud), s_own = s_dev || as || in_pin(m, us);
  char w[96];
  snprintf(w, sizeof(w), "%s %s2%s %zu B", blocking ? "hipMemcpy" : "hipMemcpyAsync", s_dev ? "D" : as || in_pin(m, us) ? "P" : "H",
           d_dev ? "D" : ad || in_pin(m, ud) ? "P" : "H", n);
  const uint32_t op = new_op(m, s, w, site);
  bool ok = true;
  if (d_own) { ad = range(m, op, dst, n, "destination"); ok = ok && ad; }
  if (s_own) { as = range(m, op, src, n, "source"); ok = ok && as; }
  if (ok) {
    if (as) touch(m, as, s, op, us - as->base, n, false);
    if (ad) touch(m, ad, s, op, ud - ad->base, n, true);
    if (s_dev && ad && !d_dev && !blocking) { /* device -> page-locked: poison now, the bytes when the host synchronises behind it */
      Pending p;
      p.op = op; p.sidx = s->idx; p.epoch = s->clock[s->idx]; p.download = true; p.host = ud; p.len = n; p.halloc = ad; p.hserial = ad->serial;
      p.bytes.assign((const uint8_t *)src, (const uint8_t *)src + n);
      memset(dst, HM_POISON, n);
      rewatch(m, ud, n);
      m.pending.push_back(std::move(p));
    } else {
      memmove(dst, src, n);
      note_written(m, ad, dst, n);
      if (as && !s_dev && d_dev && !blocking) { /* page-locked -> device: the source is the caller's to keep until it has synchronised */
        Pending p;
        p.op = op; p.sidx = s->idx; p.epoch = s->clock[s->idx]; p.download = false; p.host = us; p.len = n; p.halloc = as; p.hserial = as->serial;
        p.hash = hash_bytes((const uint8_t *)src, n);
        m.pending.push_back(std::move(p));
      }
    }
  }
  /* the blocking form, and a copy from device to pageable memory, return when the bytes have arrived */
  if (blocking || (s_dev && !d_own)) sync_stream(m, s);
  return hipSuccess;
}

struct Reach {
  Alloc *a;
  std::string via;
};
void scan_words(Model &m, const uint8_t *p, size_t n, std::vector<Reach> &out, const std::string &what) {
  for (size_t i = 0; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, p + i, 8);
    if (!in_dev(m, (uintptr_t)w) && !in_pin(m, (uintptr_t)w)) continue;
    Alloc *a = find(m, (uintptr_t)w);
    if (a) out.push_back(Reach{a, "the word at +" + std::to_string(i) + " of " + what});
    else m.n_stale++;
  }
}

void launch(Model &m, const std::string &name, const std::string &where, void *stream, const hm_arg *args, int nargs, const void *site) {
  StreamM *s = stream_of(m, (hipStream_t)stream);
  m.n_launch++;
  if (!s || !s->live) {
    hazard(m, "H2", ~0u, ~0u, nullptr, "launch of " + name + " on a stream that does not exist (" + where + ")");
    return;
  }
  const uint32_t op = new_op(m, s, "launch " + name, site, where);
  m.cur_s = s;
  m.cur_op = op;
  for (auto &e : m.effects) /* a kernel whose effect says exactly what it touches needs no footprint from its arguments */
    if (e.exact && name.find(e.name) != std::string::npos) {
      e.fn(args, nargs);
      m.cur_s = nullptr;
      return;
    }
  bool ok = true;
  std::vector<std::pair<Reach, bool>> direct; /* allocation, written */
  std::vector<Reach> reached;
  for (int i = 0; i < nargs; i++) {
    const hm_arg &a = args[i];
    const std::string an = "argument " + std::to_string(i);
    if (a.kind == HM_ARG_SCALAR) continue;
    if (a.kind == HM_ARG_BYTES) {
      scan_words(m, (const uint8_t *)a.p, a.n, reached, an);
      continue;
    }
    if (!a.p) continue;
    Alloc *al = range(m, op, a.p, 1, a.kind == HM_ARG_CONST_PTR ? "pointer argument (read)" : "pointer argument");
    if (!al) { ok = false; continue; }
    direct.emplace_back(Reach{al, an}, a.kind == HM_ARG_PTR);
    /* one level down: the words behind the pointer (job records, destination lists, tables of a set) */
    if (al->may_hold_addresses) scan_words(m, (const uint8_t *)a.p, al->base + al->size - (uintptr_t)a.p, reached, "what " + an + " points at");
  }
  { /* ... and one level below what the structs and the pointers named */
    std::map<Alloc *, std::string> first;
    for (const Reach &r : reached) first.emplace(r.a, r.via);
    for (auto &kv : first)
      if (kv.first->may_hold_addresses) scan_words(m, (const uint8_t *)kv.first->base, kv.first->size, reached, "the allocation of " + std::to_string(kv.first->size) + " bytes reached through " + kv.second);
  }
  std::map<Alloc *, std::pair<bool, std::string>> foot;
  for (const Reach &r : reached) foot.emplace(r.a, std::make_pair(true, r.via)); /* reached through a word: nothing says it is only read */
  for (auto &d : direct) foot.emplace(d.first.a, std::make_pair(d.second, d.first.via));
  for (auto &kv : foot) touch(m, kv.first, s, op, 0, kv.first->size, kv.second.first, kv.second.second.c_str());
  if (ok)
    for (auto &e : m.effects)
      if (!e.exact && name.find(e.name) != std::string::npos) e.fn(args, nargs);
  m.cur_s = nullptr;
}

/* ---- the three kernels that only move bytes: their effects are exact (what they touch, byte for byte) and move the bytes ---- */
bool scalar_u32(const hm_arg &a, uint32_t *v) {
  if (a.kind != HM_ARG_SCALAR || a.n != 4) return false;
  memcpy(v, a.p, 4);
  return true;
}
/* a range of the running launch: inside a live allocation (recorded, true) or H2 */
bool effect_touch(Model &m, const void *p, size_t n, bool write, const char *role) {
  if (!n) return true;
  Alloc *a = range(m, m.cur_op, p, n, role);
  if (!a) return false;
  touch(m, a, m.cur_s, m.cur_op, (uintptr_t)p - a->base, n, write);
  return true;
}
struct Row {
  uintptr_t p;
  size_t n;
  bool write;
};
/* many rows at once: neighbours are merged first, so that a sorted batch is a handful of ranges */
void effect_touch_rows(Model &m, std::vector<Row> &rows, std::vector<char> *good) {
  std::vector<size_t> order(rows.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return rows[x].write != rows[y].write ? rows[x].write < rows[y].write : rows[x].p < rows[y].p; });
  for (size_t i = 0; i < order.size();) {
    size_t j = i + 1;
    uintptr_t lo = rows[order[i]].p, hi = lo + rows[order[i]].n;
    Alloc *a = find(m, lo);
    while (j < order.size() && rows[order[j]].write == rows[order[i]].write && rows[order[j]].p <= hi && a && rows[order[j]].p + rows[order[j]].n <= a->base + a->size) {
      hi = std::max(hi, rows[order[j]].p + rows[order[j]].n);
      j++;
    }
    const bool ok = effect_touch(m, (const void *)lo, hi - lo, rows[order[i]].write, rows[order[i]].write ? "destination row(s)" : "source row(s)");
    for (size_t k = i; k < j; k++) (*good)[order[k]] = ok;
    i = j;
  }
}

/* nrq_ctl_copy_kernel(uint4 *dst, const uint4 *src, uint32_t n16) */
void ctl_copy_effect(const hm_arg *a, int n) {
  Model &m = M();
  uint32_t n16;
  if (n != 3 || !scalar_u32(a[2], &n16)) { hazard(m, "H2", ~0u, m.cur_op, nullptr, "nrq_ctl_copy_kernel: unexpected arguments"); return; }
  const size_t bytes = (size_t)n16 * 16;
  const bool rs = effect_touch(m, a[1].p, bytes, false, "source"), rd = effect_touch(m, a[0].p, bytes, true, "destination");
  if (rs && rd) {
    memmove((void *)a[0].p, a[1].p, bytes);
    note_written(m, find(m, (uintptr_t)a[0].p), a[0].p, bytes);
  }
}
/* nrq_scatter_kernel(const uint8_t *blob, uint32_t T, const uint64_t *dst, uint32_t n): row k of blob to dst[k] (0 = drop) */
void scatter_effect(const hm_arg *a, int na) {
  Model &m = M();
  uint32_t T, n;
  if (na != 4 || !scalar_u32(a[1], &T) || !scalar_u32(a[3], &n)) { hazard(m, "H2", ~0u, m.cur_op, nullptr, "nrq_scatter_kernel: unexpected arguments"); return; }
  if (!effect_touch(m, a[2].p, (size_t)n * 8, false, "destination list")) return;
  const uint64_t *dst = (const uint64_t *)a[2].p;
  std::vector<Row> rows;
  for (uint32_t k = 0; k < n; k++)
    if (dst[k]) {
      rows.push_back(Row{(uintptr_t)a[0].p + (size_t)k * T, T, false});
      rows.push_back(Row{(uintptr_t)dst[k], T, true});
    }
  std::vector<char> good(rows.size(), 0);
  effect_touch_rows(m, rows, &good);
  for (size_t i = 0; i + 1 < rows.size(); i += 2)
    if (good[i] && good[i + 1]) {
      memmove((void *)rows[i + 1].p, (const void *)rows[i].p, T);
      note_written(m, find(m, rows[i + 1].p), (const void *)rows[i + 1].p, T);
    }
}
/* nrq_move_rows_kernel(const uint64_t *pairs, uint32_t T, uint32_t n): row k from pairs[2k] to pairs[2k + 1] */
void move_rows_effect(const hm_arg *a, int na) {
  Model &m = M();
  uint32_t T, n;
  if (na != 3 || !scalar_u32(a[1], &T) || !scalar_u32(a[2], &n)) { hazard(m, "H2", ~0u, m.cur_op, nullptr, "nrq_move_rows_kernel: unexpected arguments"); return; }
  if (!effect_touch(m, a[0].p, (size_t)n * 16, false, "pair list")) return;
  const uint64_t *pr = (const uint64_t *)a[0].p;
  std::vector<Row> rows;
  for (uint32_t k = 0; k < n; k++)
    if (pr[2 * k] && pr[2 * k + 1]) {
      rows.push_back(Row{(uintptr_t)pr[2 * k], T, false});
      rows.push_back(Row{(uintptr_t)pr[2 * k + 1], T, true});
    }
  std::vector<char> good(rows.size(), 0);
  effect_touch_rows(m, rows, &good);
  for (size_t i = 0; i + 1 < rows.size(); i += 2)
    if (good[i] && good[i + 1]) {
      memmove((void *)rows[i + 1].p, (const void *)rows[i].p, T);
      note_written(m, find(m, rows[i + 1].p), (const void *)rows[i + 1].p, T);
    }
}

void json_str(std::string &o, const std::string &s) {
  o += '"';
  for (char c : s) {
    if (c == '"' || c == '\\') { o += '\\'; o += c; }
    else if ((unsigned char)c < 0x20) o += ' ';
    else o += c;
  }
  o += '"';
}
void json_op(Model &m, std::string &o, uint32_t op) {
  if (op == ~0u || op >= m.ops.size()) { o += "null"; return; }
  const OpInfo &i = m.ops[op];
  o += "{\"what\":"; json_str(o, i.what);
  o += ",\"stream\":" + std::to_string(i.sidx) + ",\"n\":" + std::to_string(i.epoch) + ",\"site\":";
  json_str(o, i.where.empty() ? site_name(i.site) : i.where + " " + site_name(i.site));
  o += "}";
}

} // namespace

#define SITE __builtin_return_address(0)

extern "C" {

/* ---------------------------------------------------------------- the model's own interface */
void hm_model_launch(const void *fn, const char *file, int line, void *stream, const unsigned grid[3], const hm_arg *args, int nargs) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  for (int i = 0; i < 3; i++) m.cur_grid[i] = grid ? grid[i] : 1u;
  auto it = m.kernels.find(fn);
  if (it == m.kernels.end()) m.n_unnamed++;
  const char *base = file ? (strrchr(file, '/') ? strrchr(file, '/') + 1 : file) : "?";
  launch(m, it == m.kernels.end() ? "(unregistered kernel)" : it->second, std::string(base) + ":" + std::to_string(line), stream, args, nargs, SITE);
}
void hm_launch_named(const char *name, void *stream, const hm_arg *args, int nargs) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  launch(m, name ? name : "?", "", stream, args, nargs, SITE);
}
void hm_set_effect(const char *name_part, hm_effect_fn fn, int exact) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  m.effects.push_back(Model::Effect{name_part, fn, exact != 0});
}
int hm_effect_touch_tail(const void *p, int write) {
  Model &m = M();
  Alloc *a = m.cur_s ? find(m, (uintptr_t)p) : nullptr;
  if (!a) return m.cur_s ? effect_touch(m, p, 1, write != 0, "buffer") : 0;
  return effect_touch(m, p, a->base + a->size - (uintptr_t)p, write != 0, "buffer");
}
uint64_t hm_effect_base(const void *p) {
  Model &m = M(); /* (called from an effect: the model is locked) */
  Alloc *a = m.cur_s ? find(m, (uintptr_t)p) : nullptr;
  return a ? (uint64_t)a->base : 0;
}
void hm_effect_wrote(const void *p, size_t n) {
  Model &m = M();
  if (m.cur_s) note_written(m, find(m, (uintptr_t)p), p, n);
}
void hm_effect_grid(unsigned out[3]) {
  Model &m = M();
  for (int i = 0; i < 3; i++) out[i] = m.cur_grid[i];
}
int hm_effect_touch(const void *p, size_t n, int write) {
  Model &m = M(); /* (called from an effect: the model is locked and knows the launch) */
  return m.cur_s ? effect_touch(m, p, n, write != 0, write ? "written range" : "read range") : 0;
}
uint64_t hm_hazard_count(void) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  return m.hazards.size();
}
void hm_hazards_clear(void) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  m.hazards.clear();
}
size_t hm_hazards_json(char *buf, size_t cap) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  std::string o = "[";
  for (size_t i = 0; i < m.hazards.size(); i++) {
    const Hazard &h = m.hazards[i];
    if (i) o += ",";
    o += "{\"kind\":"; json_str(o, h.kind);
    o += ",\"detail\":"; json_str(o, h.detail);
    o += ",\"first\":"; json_op(m, o, h.op_a);
    o += ",\"second\":"; json_op(m, o, h.op_b);
    char a[160];
    snprintf(a, sizeof(a), ",\"allocation\":{\"base\":%llu,\"size\":%zu,\"kind\":%d}}", (unsigned long long)h.base, h.size, h.akind);
    o += a;
  }
  o += "]";
  if (buf && cap) {
    const size_t n = std::min(cap - 1, o.size());
    memcpy(buf, o.data(), n);
    buf[n] = 0;
  }
  return o.size() + 1;
}
void hm_counters(uint64_t out[8]) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  out[0] = m.ops.size(); out[1] = m.n_launch; out[2] = m.n_copy; out[3] = m.n_unrec; out[4] = m.live.size(); out[5] = m.n_stale;
  out[6] = m.pending.size(); out[7] = m.n_unnamed;
}
int hm_block_of(const void *p, uint64_t *base, uint64_t *size, int *kind) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  Alloc *a = find(m, (uintptr_t)p);
  if (!a) return 0;
  if (base) *base = a->base;
  if (size) *size = a->size;
  if (kind) *kind = a->kind;
  return 1;
}
int hm_pending_on(const void *p) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  Alloc *a = find(m, (uintptr_t)p);
  return a ? pending_on(m, a) : -1;
}
int hm_pending_total(void) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  int n = 0;
  for (auto &kv : m.live) n += pending_on(m, kv.second.get());
  return n;
}

/* ---------------------------------------------------------------- what the compiler's registration code calls */
void **__hipRegisterFatBinary(const void *) {
  static void *handle[2];
  static bool once = false;
  if (!once) {
    once = true;
    hm_set_effect("nrq_ctl_copy_kernel", ctl_copy_effect, 1);
    hm_set_effect("nrq_scatter_kernel", scatter_effect, 1);
    hm_set_effect("nrq_move_rows_kernel", move_rows_effect, 1);
  }
  return handle;
}
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  m.kernels[host_fn] = device_name ? device_name : "?";
}
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *, dim3 *, size_t *, hipStream_t *) { return hipSuccess; }
/* every launch of the host layer goes through the hook; the kernels' host stubs still name this one */
hipError_t hipLaunchKernel(const void *, dim3, dim3, void **, size_t, hipStream_t) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  hazard(m, "H2", ~0u, ~0u, nullptr, "a launch went past the hook (hipLaunchKernel): its footprint is unknown");
  return hipErrorUnknown;
}

/* ---------------------------------------------------------------- device, errors */
hipError_t hipGetDeviceCount(int *n) { if (n) *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t a, int) {
  if (!v) return hipErrorInvalidValue;
  *v = a == hipDeviceAttributeMultiprocessorCount ? 256 : 0; /* (the compute units of an MI355X) */
  return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return err_name(e); }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }

/* ---------------------------------------------------------------- memory */
hipError_t hipMalloc(void **out, size_t bytes) {
  if (!out) return hipErrorInvalidValue;
  *out = nullptr;
  if (!bytes) return hipSuccess;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  void *p = carve(m, false, bytes);
  if (!p) return hipErrorOutOfMemory;
  add_alloc(m, (uintptr_t)p, bytes, K_DEV, SITE);
  *out = p;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  if (!p) return hipSuccess;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  sync_device(m); /* (device-wide synchronisation: the library relies on it) */
  auto it = m.live.find((uintptr_t)p);
  if (it == m.live.end() || it->second->kind != K_DEV) {
    const uint32_t op = new_op(m, m.streams[0].get(), "hipFree", SITE);
    hazard(m, "H2", ~0u, op, find_dead(m, (uintptr_t)p), find_dead(m, (uintptr_t)p) ? "hipFree of an allocation that was already released" : "hipFree of an address that is no allocation");
    return hipErrorInvalidValue;
  }
  retire(m, it->second.get());
  return hipSuccess;
}
hipError_t hipHostMalloc(void **out, size_t bytes, unsigned) {
  if (!out) return hipErrorInvalidValue;
  *out = nullptr;
  if (!bytes) return hipSuccess;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  void *p = carve(m, true, bytes);
  if (!p) return hipErrorOutOfMemory;
  add_alloc(m, (uintptr_t)p, bytes, K_PIN, SITE);
  *out = p;
  return hipSuccess;
}
static hipError_t release_host(void *p, int kind, const char *what, const void *site) {
  if (!p) return hipSuccess;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  auto it = m.live.find((uintptr_t)p);
  if (it == m.live.end() || it->second->kind != kind) {
    const uint32_t op = new_op(m, m.streams[0].get(), what, site);
    hazard(m, "H2", ~0u, op, find_dead(m, (uintptr_t)p), std::string(what) + " of an address that is no such allocation (or was already released)");
    return kind == K_REG ? hipErrorHostMemoryNotRegistered : hipErrorInvalidValue;
  }
  Alloc *a = it->second.get();
  /* NOT a synchronisation (hip_model.h): whatever still touches the allocation is reported */
  for (const Access &x : a->acc)
    if (!done_for_host(m, x.sidx, x.epoch)) {
      const uint32_t op = new_op(m, m.streams[0].get(), what, site);
      hazard(m, "H3", x.op, op, a, std::string(what) + " while an operation the host has not synchronised behind touches the allocation");
      break;
    }
  retire(m, a);
  return hipSuccess;
}
hipError_t hipHostFree(void *p) { return release_host(p, K_PIN, "hipHostFree", SITE); }
hipError_t hipHostUnregister(void *p) { return release_host(p, K_REG, "hipHostUnregister", SITE); }
hipError_t hipHostRegister(void *p, size_t bytes, unsigned) {
  if (!p || !bytes) return hipErrorInvalidValue;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  if (find(m, (uintptr_t)p) || find(m, (uintptr_t)p + bytes - 1)) return hipErrorHostMemoryAlreadyRegistered;
  auto it = m.live.lower_bound((uintptr_t)p);
  if (it != m.live.end() && it->first < (uintptr_t)p + bytes) return hipErrorHostMemoryAlreadyRegistered;
  add_alloc(m, (uintptr_t)p, bytes, K_REG, SITE);
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  Alloc *a = find(m, (uintptr_t)h);
  if (!d || !a || a->kind == K_DEV) return hipErrorInvalidValue;
  *d = h;
  return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *attr, const void *p) {
  if (!attr) return hipErrorInvalidValue;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  memset(attr, 0, sizeof(*attr));
  Alloc *a = find(m, (uintptr_t)p);
  attr->type = !a ? hipMemoryTypeUnregistered : a->kind == K_DEV ? hipMemoryTypeDevice : hipMemoryTypeHost;
  if (a) {
    attr->devicePointer = const_cast<void *>(p);
    attr->hostPointer = a->kind == K_DEV ? nullptr : const_cast<void *>(p);
  }
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t st) { return do_copy(dst, src, n, kind, st, false, SITE); }
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) { return do_copy(dst, src, n, kind, nullptr, true, SITE); }
hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t st) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  StreamM *s = stream_of(m, st);
  if (!s || !s->live) return hipErrorInvalidResourceHandle;
  if (!n) return hipSuccess;
  m.n_copy++;
  char w[64];
  snprintf(w, sizeof(w), "hipMemsetAsync %zu B", n);
  const uint32_t op = new_op(m, s, w, SITE);
  Alloc *a = range(m, op, dst, n, "destination");
  if (!a) return hipSuccess; /* (reported; the runtime's own answer to a bad range is not the point here) */
  touch(m, a, s, op, (uintptr_t)dst - a->base, n, true);
  memset(dst, value, n);
  return hipSuccess;
}

/* ---------------------------------------------------------------- streams and events */
hipError_t hipStreamCreateWithFlags(hipStream_t *out, unsigned) {
  if (!out) return hipErrorInvalidValue;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  m.streams.emplace_back(new StreamM());
  StreamM *s = m.streams.back().get();
  s->idx = (int)m.streams.size() - 1;
  s->clock.assign(s->idx + 1, 0);
  *out = (hipStream_t)s;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t h) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  StreamM *s = stream_of(m, h);
  if (!s || !h || !s->live) return hipErrorInvalidResourceHandle;
  s->live = false; /* (its work stays pending until someone synchronises with the device: the object stays, with its clock) */
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t h) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  StreamM *s = stream_of(m, h);
  if (!s || !s->live) return hipErrorInvalidResourceHandle;
  sync_stream(m, s);
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  sync_device(m);
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t h, hipEvent_t ev, unsigned) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  StreamM *s = stream_of(m, h);
  EventM *e = event_of(m, ev);
  if (!s || !s->live || !e || !e->live) return hipErrorInvalidResourceHandle;
  if (e->recorded) vc_join(s->clock, e->vc);
  else m.n_unrec++; /* orders nothing, as in HIP */
  return hipSuccess;
}
static hipError_t event_new(hipEvent_t *out) {
  if (!out) return hipErrorInvalidValue;
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  m.events.emplace_back(new EventM());
  *out = (hipEvent_t)m.events.back().get();
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *out) { return event_new(out); }
hipError_t hipEventCreateWithFlags(hipEvent_t *out, unsigned) { return event_new(out); }
hipError_t hipEventDestroy(hipEvent_t ev) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  EventM *e = event_of(m, ev);
  if (!e || !e->live) return hipErrorInvalidResourceHandle;
  e->live = false;
  for (size_t i = 0; i < m.events.size(); i++)
    if (m.events[i].get() == e) { m.events.erase(m.events.begin() + i); break; }
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t h) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  StreamM *s = stream_of(m, h);
  EventM *e = event_of(m, ev);
  if (!s || !s->live || !e || !e->live) return hipErrorInvalidResourceHandle;
  vc_join(s->clock, m.host);
  e->vc = s->clock;
  e->recorded = true;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  EventM *e = event_of(m, ev);
  if (!e || !e->live) return hipErrorInvalidResourceHandle;
  if (e->recorded) {
    vc_join(m.host, e->vc);
    host_advanced(m);
  }
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  Model &m = M();
  std::lock_guard<std::mutex> g(m.mu);
  EventM *ea = event_of(m, a), *eb = event_of(m, b);
  if (!ms || !ea || !eb) return hipErrorInvalidResourceHandle;
  if (!ea->recorded || !eb->recorded) return hipErrorInvalidResourceHandle;
  for (EventM *e : {ea, eb})
    for (size_t i = 0; i < e->vc.size(); i++)
      if (vc_at(m.host, i) < e->vc[i]) return hipErrorNotReady;
  *ms = 0.001f;
  return hipSuccess;
}

} /* extern "C" */
