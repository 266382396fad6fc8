/*
 * gf2.h -- a STAND-IN for the bit-matrix header of the reference's field library (see octmat.h: not upstream oblas, pinned
 * commit unknown, written from the reference's call sites: lib/wrkmat.c:12,27,62,69,81,83,90,100 and the gf2row / gf2el
 * macros of include/wrkmat.h, which read `bits` and `stride` directly).
 *
 * Row r starts at bits + r * stride (stride in 32-bit words); column j is bit j % 32 of word j / 32.
 */
#ifndef REFSHIM_GF2_H
#define REFSHIM_GF2_H

#include <stddef.h>
#include <stdint.h>

typedef struct {
  size_t rows;
  size_t cols;
  size_t stride;
  uint32_t *bits;
} gf2mat;

gf2mat *gf2mat_new(size_t rows, size_t cols); /* all zero */
void gf2mat_free(gf2mat *m);
int gf2mat_get(const gf2mat *m, size_t i, size_t j);
void gf2mat_set(gf2mat *m, size_t i, size_t j, int b);
/* row i of a ^= row j of b */
void gf2mat_xor(gf2mat *a, const gf2mat *b, size_t i, size_t j);
/* dst[x] = bit x of row i, as a byte 0 or 1, for every column x */
void gf2mat_fill(const gf2mat *m, size_t i, uint8_t *dst);

#endif
