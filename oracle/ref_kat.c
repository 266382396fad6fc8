/*
 * ref_kat.c -- one driver, two builds (oracle/Makefile): `_ref/ref_kat` links the REFERENCE's own lib/*.c (read in place,
 * over the stand-in field library of oracle/refshim/), `_ref/ref_kat_hip` links this repository's libnanorq_hip.so.  Both
 * expose the same public API (nanorq.h, io.h), which is all this file uses, so the same cases give records that must be
 * equal line for line.  tools/gen_ref_kat.py turns the first build's records into tests/golden/ref_kat.json; the tests
 * (tests/test_ref_kat.py, tests/test_gpu_ref_kat.py) hold the second build, and the oracle, to that file.
 *
 *   ref_kat [--host] [CASEFILE]        cases from CASEFILE or stdin, records to stdout
 *
 * A case is one line of blank-separated words; every object is given as  len T K Z Al ex  (ex = 0: nanorq_encoder_new(len, T,
 * Al), K and Z ignored; ex = 1: nanorq_encoder_new_ex) and its payload is byte i = ((uint32) i * 2654435761) >> 24:
 *
 *   params ID len T K Z Al ex
 *   encode ID len T K Z Al ex PRECALC SYMS...         SYMS:  sbn:esi  or  sbn:lo-hi (inclusive)
 *   decode ID len T K Z Al ex MAXESI OPS...           MAXESI: -1 = leave the default
 *       OPS:  a<sbn>:<esi> | a<sbn>:<lo>-<hi>   add the symbol(s); the payload comes from an encoder of the same library
 *             r<sbn>                            nanorq_repair_block now
 *             n<sbn>                            nanorq_num_missing / nanorq_num_repair now
 *       after the script, for every block: the counts, repair_block, repair_block again, the missing count; then the
 *       output buffer, which was filled with 0x3C before the first symbol.
 *
 * --host: nothing that needs the solver is called (no generate_symbols, no repair_block, no repair symbol is encoded): source
 * payloads are the unsolved encoder's copies, repair payloads are 0xA5 filler.  The add_symbol codes, the counts and where
 * source symbols are written through do not depend on a solver, so this mode runs where there is no GPU.
 *
 * Records are text: "begin ID" before anything is called for a case (so a reader knows which case a dead process was in),
 * then one line per observation, then "end ID"; stdout is flushed after every case.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <nanorq.h>

static int host_only;

struct object {
  size_t len;
  unsigned T, K, Z, Al, ex;
};

static uint8_t *payload(size_t len) {
  uint8_t *p = malloc(len ? len : 1);
  for (size_t i = 0; i < len; i++)
    p[i] = (uint8_t)(((uint32_t)i * 2654435761u) >> 24);
  return p;
}

static nanorq *new_encoder(const struct object *o) {
  if (o->ex)
    return nanorq_encoder_new_ex(o->len, (uint16_t)o->T, (uint16_t)o->K, (uint16_t)o->Z, (uint8_t)o->Al);
  return nanorq_encoder_new(o->len, (uint16_t)o->T, (uint8_t)o->Al);
}

static void put_hex(const uint8_t *p, size_t n) {
  static const char dig[] = "0123456789abcdef";
  for (size_t i = 0; i < n; i++) {
    putchar(dig[p[i] >> 4]);
    putchar(dig[p[i] & 15]);
  }
}

/* the next word of the case line, NULL at its end */
static char *word(char **line) {
  char *s = *line;
  while (*s == ' ' || *s == '\t' || *s == '\n' || *s == '\r')
    s++;
  if (!*s)
    return NULL;
  char *e = s;
  while (*e && *e != ' ' && *e != '\t' && *e != '\n' && *e != '\r')
    e++;
  if (*e)
    *e++ = 0;
  *line = e;
  return s;
}

static int read_object(char **line, struct object *o) {
  char *w[6];
  for (int i = 0; i < 6; i++)
    if (!(w[i] = word(line)))
      return 0;
  o->len = (size_t)strtoull(w[0], NULL, 10);
  o->T = (unsigned)strtoul(w[1], NULL, 10);
  o->K = (unsigned)strtoul(w[2], NULL, 10);
  o->Z = (unsigned)strtoul(w[3], NULL, 10);
  o->Al = (unsigned)strtoul(w[4], NULL, 10);
  o->ex = (unsigned)strtoul(w[5], NULL, 10);
  return 1;
}

/* "sbn:esi" or "sbn:lo-hi" */
static int read_syms(const char *s, unsigned *sbn, uint32_t *lo, uint32_t *hi) {
  char *e;
  *sbn = (unsigned)strtoul(s, &e, 10);
  if (*e != ':')
    return 0;
  *lo = *hi = (uint32_t)strtoul(e + 1, &e, 10);
  if (*e == '-')
    *hi = (uint32_t)strtoul(e + 1, &e, 10);
  return *e == 0 && *hi >= *lo && *sbn < 256;
}

static void facts(nanorq *rq) {
  size_t Z = nanorq_blocks(rq);
  printf("new ok common=%016" PRIx64 " scheme=%08" PRIx32 " F=%zu T=%zu Z=%zu maxblocks=%zu\nks", nanorq_oti_common(rq),
         nanorq_oti_scheme_specific(rq), nanorq_transfer_length(rq), nanorq_symbol_size(rq), Z, nanorq_max_blocks(rq));
  for (size_t b = 0; b < Z; b++)
    printf(" %zu", nanorq_block_symbols(rq, (uint8_t)b));
  printf("\n");
}

static void run_params(const struct object *o) {
  nanorq *rq = new_encoder(o);
  if (!rq) {
    printf("new null\n");
    return;
  }
  facts(rq);
  nanorq_free(rq);
}

/* an encoder over the payload; *io reads it */
static nanorq *open_encoder(const struct object *o, uint8_t **src, struct ioctx **io) {
  nanorq *rq = new_encoder(o);
  if (!rq)
    return NULL;
  *src = payload(o->len);
  *io = ioctx_from_mem(*src, o->len);
  return rq;
}

static void run_encode(const struct object *o, char **line) {
  char *w = word(line);
  int precalc = w ? atoi(w) : 0;
  uint8_t *src = NULL;
  struct ioctx *io = NULL;
  nanorq *rq = open_encoder(o, &src, &io);
  if (!rq) {
    printf("new null\n");
    return;
  }
  facts(rq);
  size_t T = nanorq_symbol_size(rq), Z = nanorq_blocks(rq);
  if (precalc)
    printf("precalc %d\n", (int)nanorq_precalculate(rq));
  for (size_t b = 0; b < Z; b++)
    printf("gen %zu %d\n", b, (int)nanorq_generate_symbols(rq, (uint8_t)b, io));
  uint8_t *sym = malloc(T);
  while ((w = word(line))) {
    unsigned sbn;
    uint32_t lo, hi;
    if (!read_syms(w, &sbn, &lo, &hi)) {
      printf("bad %s\n", w);
      break;
    }
    for (uint32_t esi = lo;; esi++) {
      memset(sym, 0x3C, T);
      size_t n = nanorq_encode(rq, sym, esi, (uint8_t)sbn, io);
      printf("sym %u %" PRIu32 " %zu ", sbn, esi, n);
      put_hex(sym, T);
      printf("\n");
      if (esi == hi)
        break;
    }
  }
  free(sym);
  nanorq_free(rq);
  io->destroy(io);
  free(src);
}

static void run_decode(const struct object *o, char **line) {
  char *w = word(line);
  long max_esi = w ? strtol(w, NULL, 10) : -1;
  uint8_t *src = NULL;
  struct ioctx *io = NULL;
  nanorq *enc = open_encoder(o, &src, &io);
  if (!enc) {
    printf("new null\n");
    return;
  }
  nanorq *dec = nanorq_decoder_new(nanorq_oti_common(enc), nanorq_oti_scheme_specific(enc));
  if (!dec) {
    printf("decoder null\n");
    nanorq_free(enc);
    io->destroy(io);
    free(src);
    return;
  }
  facts(dec);
  size_t T = nanorq_symbol_size(dec), Z = nanorq_blocks(dec);
  if (max_esi >= 0)
    printf("setmax %d\n", (int)nanorq_set_max_esi(dec, (uint32_t)max_esi));
  uint8_t *out = malloc(o->len ? o->len : 1), *sym = malloc(T);
  memset(out, 0x3C, o->len);
  struct ioctx *oio = ioctx_from_mem(out, o->len);
  char solved[256] = {0};
  while ((w = word(line))) {
    unsigned sbn;
    uint32_t lo, hi;
    if (w[0] == 'r' || w[0] == 'n') {
      sbn = (unsigned)strtoul(w + 1, NULL, 10) & 255;
      if (w[0] == 'n')
        printf("num %u %zu %zu\n", sbn, nanorq_num_missing(dec, (uint8_t)sbn), nanorq_num_repair(dec, (uint8_t)sbn));
      else if (!host_only)
        printf("rep %u %d\n", sbn, (int)nanorq_repair_block(dec, oio, (uint8_t)sbn));
      continue;
    }
    if (w[0] != 'a' || !read_syms(w + 1, &sbn, &lo, &hi)) {
      printf("bad %s\n", w);
      break;
    }
    for (uint32_t esi = lo;; esi++) {
      /* the payload: what an encoder of this library sends for (sbn, esi); filler where it sends nothing (a block the
       * object does not have) or where it would need the solver and there is none */
      memset(sym, 0xA5, T);
      if (sbn < Z && (!host_only || esi < nanorq_block_symbols(enc, (uint8_t)sbn))) {
        if (!host_only && !solved[sbn]) {
          solved[sbn] = 1;
          if (!nanorq_generate_symbols(enc, (uint8_t)sbn, io))
            printf("gen %u 0\n", sbn);
        }
        if (nanorq_encode(enc, sym, esi, (uint8_t)sbn, io) != T)
          printf("short %u %" PRIu32 "\n", sbn, esi);
      }
      printf("add %u %" PRIu32 " %d\n", sbn, esi, nanorq_decoder_add_symbol(dec, sym, nanorq_tag((uint8_t)sbn, esi), oio));
      if (esi == hi)
        break;
    }
  }
  for (size_t b = 0; b < Z; b++) {
    size_t nm = nanorq_num_missing(dec, (uint8_t)b), nr = nanorq_num_repair(dec, (uint8_t)b);
    if (host_only) {
      printf("final %zu %zu %zu\n", b, nm, nr);
      continue;
    }
    int v1 = (int)nanorq_repair_block(dec, oio, (uint8_t)b);
    int v2 = (int)nanorq_repair_block(dec, oio, (uint8_t)b);
    printf("final %zu %zu %zu %d %d %zu\n", b, nm, nr, v1, v2, nanorq_num_missing(dec, (uint8_t)b));
  }
  printf("out ");
  put_hex(out, o->len);
  printf("\n");
  nanorq_free(dec);
  nanorq_free(enc);
  oio->destroy(oio);
  io->destroy(io);
  free(sym);
  free(out);
  free(src);
}

int main(int argc, char **argv) {
  FILE *in = stdin;
  for (int a = 1; a < argc; a++) {
    if (!strcmp(argv[a], "--host"))
      host_only = 1;
    else if (!(in = fopen(argv[a], "r"))) {
      fprintf(stderr, "ref_kat: cannot read %s\n", argv[a]);
      return 2;
    }
  }
  char *buf = NULL;
  size_t cap = 0;
  while (getline(&buf, &cap, in) > 0) {
    char *line = buf, *kind = word(&line), *id = kind ? word(&line) : NULL;
    struct object o;
    if (!kind || kind[0] == '#')
      continue;
    if (!id || !read_object(&line, &o)) {
      fprintf(stderr, "ref_kat: malformed case line\n");
      return 2;
    }
    printf("begin %s %s\n", id, kind);
    fflush(stdout);
    if (!strcmp(kind, "params"))
      run_params(&o);
    else if (!strcmp(kind, "encode") && !host_only)
      run_encode(&o, &line);
    else if (!strcmp(kind, "decode"))
      run_decode(&o, &line);
    else
      printf("skipped\n");
    printf("end %s\n", id);
    fflush(stdout);
  }
  free(buf);
  return 0;
}
