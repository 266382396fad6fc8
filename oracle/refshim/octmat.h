/*
 * octmat.h -- a STAND-IN for the octet-matrix header of the reference's field library (its `deps/oblas` submodule, which is
 * empty in the reference tree; the pinned commit is unknown).  This is not upstream oblas: it is this project's own, scalar
 * restatement of the contract the reference's call sites imply (lib/nanorq.c wherever om_* is used, lib/precode.c:60-80 and
 * :233-251, lib/wrkmat.c).  It exists so that the reference's own library sources can be compiled and run as
 * the source of known answers (oracle/ref_kat.c, tests/golden/ref_kat.json).  Test infrastructure only.
 *
 * The contract: a row-major byte matrix whose rows are `cols_al` bytes apart, cols_al = cols rounded up to 32; om_resize
 * hands out zero-filled storage (the reference relies on that for its padding, LDPC and HDPC rows) and forgets what the
 * matrix held before.
 */
#ifndef REFSHIM_OCTMAT_H
#define REFSHIM_OCTMAT_H

#include <stddef.h>
#include <stdint.h>

#define OCTMAT_ALIGN 32

typedef struct {
  uint8_t *data;
  size_t rows;
  size_t cols;
  size_t cols_al;
} octmat;

#define OM_INITIAL {NULL, 0, 0, 0}

#define om_P(m) ((m).data)
#define om_R(m, r) ((m).data + (size_t)(r) * (m).cols_al)
#define om_A(m, r, c) (om_R(m, r)[c])

void om_resize(octmat *m, size_t rows, size_t cols);
void om_destroy(octmat *m);

#endif
