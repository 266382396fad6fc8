/*
 * refshim.c -- the one source file of the STAND-IN for the reference's absent field library (octmat.h, oblas.h, gf2.h of
 * this directory: not upstream oblas, pinned commit unknown, this project's own code written from the reference's call
 * sites).  Scalar and meant to be read, not to be fast.
 *
 * With -DREFSHIM_SELFTEST the file has a main() that prints the three tables and what the four row kernels do at the row
 * lengths 1, 31, 32 and 33 (around the 32-byte row stride); tests/test_ref_kat.py checks that print-out against the
 * project's own GF(256) tables and against arithmetic modulo 0x11D done in Python, so the field does not vouch for itself.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gf2.h"
#include "oblas.h"
#include "octmat.h"

uint8_t OCT_EXP[510];
uint8_t OCT_LOG[256];
uint8_t OCT_INV[256];

__attribute__((constructor)) static void oct_tables(void) {
  unsigned x = 1;
  for (int n = 0; n < 255; n++) {
    OCT_EXP[n] = OCT_EXP[n + 255] = (uint8_t)x;
    OCT_LOG[x] = (uint8_t)n;
    x <<= 1;
    if (x & 0x100)
      x ^= 0x11D;
  }
  OCT_INV[0] = 0;
  for (int v = 1; v < 256; v++)
    OCT_INV[v] = OCT_EXP[255 - OCT_LOG[v]];
}

static uint8_t mul(uint8_t a, uint8_t b) {
  return (a && b) ? OCT_EXP[OCT_LOG[a] + OCT_LOG[b]] : 0;
}

static size_t stride_of(size_t k) {
  return (k + OCTMAT_ALIGN - 1) / OCTMAT_ALIGN * OCTMAT_ALIGN;
}

void om_resize(octmat *m, size_t rows, size_t cols) {
  m->rows = rows;
  m->cols = cols;
  m->cols_al = stride_of(cols);
  m->data = calloc(rows ? rows : 1, m->cols_al ? m->cols_al : OCTMAT_ALIGN);
  if (!m->data)
    abort();
}

void om_destroy(octmat *m) {
  free(m->data);
  m->data = NULL;
  m->rows = m->cols = m->cols_al = 0;
}

void oaxpy(uint8_t *a, const uint8_t *b, size_t i, size_t j, size_t k, uint8_t beta) {
  uint8_t *dst = a + i * stride_of(k);
  const uint8_t *src = b + j * stride_of(k);
  for (size_t x = 0; x < k; x++)
    dst[x] ^= mul(src[x], beta);
}

void oscal(uint8_t *a, size_t i, size_t k, uint8_t beta) {
  uint8_t *dst = a + i * stride_of(k);
  for (size_t x = 0; x < k; x++)
    dst[x] = mul(dst[x], beta);
}

void oswaprow(uint8_t *a, size_t i, size_t j, size_t k) {
  uint8_t *p = a + i * stride_of(k), *q = a + j * stride_of(k);
  for (size_t x = 0; x < k; x++) {
    uint8_t t = p[x];
    p[x] = q[x];
    q[x] = t;
  }
}

void oaxpy_b32(uint8_t *a, const uint32_t *bits, size_t i, size_t k, uint8_t beta) {
  uint8_t *dst = a + i * stride_of(k);
  for (size_t x = 0; x < k; x++)
    if ((bits[x / 32] >> (x % 32)) & 1)
      dst[x] ^= beta;
}

gf2mat *gf2mat_new(size_t rows, size_t cols) {
  gf2mat *m = calloc(1, sizeof *m);
  if (!m)
    abort();
  m->rows = rows;
  m->cols = cols;
  m->stride = (cols + 31) / 32;
  m->bits = calloc((rows ? rows : 1) * (m->stride ? m->stride : 1), sizeof(uint32_t));
  if (!m->bits)
    abort();
  return m;
}

void gf2mat_free(gf2mat *m) {
  if (m)
    free(m->bits);
  free(m);
}

int gf2mat_get(const gf2mat *m, size_t i, size_t j) {
  return (m->bits[i * m->stride + j / 32] >> (j % 32)) & 1;
}

void gf2mat_set(gf2mat *m, size_t i, size_t j, int b) {
  uint32_t *w = &m->bits[i * m->stride + j / 32], bit = (uint32_t)1 << (j % 32);
  *w = b ? (*w | bit) : (*w & ~bit);
}

void gf2mat_xor(gf2mat *a, const gf2mat *b, size_t i, size_t j) {
  for (size_t w = 0; w < a->stride; w++)
    a->bits[i * a->stride + w] ^= b->bits[j * b->stride + w];
}

void gf2mat_fill(const gf2mat *m, size_t i, uint8_t *dst) {
  for (size_t x = 0; x < m->cols; x++)
    dst[x] = (uint8_t)gf2mat_get(m, i, x);
}

#ifdef REFSHIM_SELFTEST
static void hex(const char *name, const uint8_t *p, size_t n) {
  printf("%s ", name);
  for (size_t x = 0; x < n; x++)
    printf("%02x", p[x]);
  printf("\n");
}

/* every byte of the matrix, padding included: a kernel that runs past k shows */
static void dump(const char *what, size_t k, const octmat *m) {
  char name[64];
  snprintf(name, sizeof name, "%s %zu", what, k);
  hex(name, m->data, m->rows * m->cols_al);
}

int main(void) {
  static const size_t lens[] = {1, 31, 32, 33};
  hex("EXP", OCT_EXP, sizeof OCT_EXP);
  hex("LOG", OCT_LOG, sizeof OCT_LOG);
  hex("INV", OCT_INV, sizeof OCT_INV);
  for (size_t t = 0; t < sizeof lens / sizeof lens[0]; t++) {
    size_t k = lens[t];
    octmat m = OM_INITIAL;
    uint32_t bits[2] = {0, 0};
    gf2mat *g = gf2mat_new(3, k);
    om_resize(&m, 4, k);
    printf("STRIDE %zu %zu\n", k, m.cols_al);
    for (size_t r = 0; r < 4; r++)
      for (size_t c = 0; c < k; c++)
        om_A(m, r, c) = (uint8_t)(r * 37 + c * 11 + 5);
    dump("INIT", k, &m);
    oaxpy(om_P(m), om_P(m), 1, 2, k, 0x53);
    dump("AXPY", k, &m);
    oscal(om_P(m), 3, k, 0xCA);
    dump("SCAL", k, &m);
    oswaprow(om_P(m), 0, 3, k);
    dump("SWAP", k, &m);
    for (size_t c = 0; c < k; c++)
      if ((c * 7 + k) % 3 == 0) {
        bits[c / 32] |= (uint32_t)1 << (c % 32);
        gf2mat_set(g, 1, c, 1);
      }
    oaxpy_b32(om_P(m), bits, 2, k, 0x8E);
    dump("AXPYB32", k, &m);
    /* the bit matrix: row 2 = row 1, expanded to bytes over row 0 of m (gf2mat_fill), then row 1 ^= row 1 leaves it empty */
    gf2mat_xor(g, g, 2, 1);
    gf2mat_fill(g, 2, om_R(m, 0));
    dump("FILL", k, &m);
    gf2mat_xor(g, g, 1, 1);
    gf2mat_set(g, 0, k - 1, 1);
    printf("GF2 %zu %zu %d %d %d\n", k, g->stride, gf2mat_get(g, 0, k - 1), gf2mat_get(g, 1, 0), gf2mat_get(g, 2, 0));
    gf2mat_free(g);
    om_destroy(&m);
  }
  return 0;
}
#endif
