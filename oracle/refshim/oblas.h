/*
 * oblas.h -- a STAND-IN for the row kernels and field tables of the reference's field library (see octmat.h: not upstream
 * oblas, pinned commit unknown, written from the reference's call sites).  Plain byte loops over GF(256) with the polynomial
 * x^8+x^4+x^3+x^2+1 (0x11D) and generator 2, the field RFC 6330 section 5.7 fixes.
 *
 * Every kernel takes the BASE pointer of an octmat and a row length k; rows are k rounded up to 32 bytes apart (the callers
 * pass om_P(m) and m.cols: lib/precode.c:7,18,20, lib/wrkmat.c:79,91,104,112).
 */
#ifndef REFSHIM_OBLAS_H
#define REFSHIM_OBLAS_H

#include <stddef.h>
#include <stdint.h>

/* OCT_EXP[n] = 2^n for n < 510 (the reference indexes up to OCT_LOG[x] + 1), OCT_LOG[2^n] = n for n < 255 (OCT_LOG[0] is
 * unused), OCT_INV[x] * x = 1 (OCT_INV[0] = 0).  Filled before main() runs. */
extern uint8_t OCT_EXP[510];
extern uint8_t OCT_LOG[256];
extern uint8_t OCT_INV[256];

/* row i of a ^= beta * row j of b */
void oaxpy(uint8_t *a, const uint8_t *b, size_t i, size_t j, size_t k, uint8_t beta);
/* row i of a *= beta */
void oscal(uint8_t *a, size_t i, size_t k, uint8_t beta);
/* rows i and j of a change places */
void oswaprow(uint8_t *a, size_t i, size_t j, size_t k);
/* a[i][x] ^= beta for every x < k whose bit is set in `bits` (32-bit words, least significant bit first) */
void oaxpy_b32(uint8_t *a, const uint32_t *bits, size_t i, size_t k, uint8_t beta);

#endif
