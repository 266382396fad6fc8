/* CPU emulation of the device-resident object layout (nanorq_amd/csrc/obj_body.h): the body nrq_obj_layout_kernel runs, called
 * for every (block, work item) in a loop, at the piece width the library would choose (or a narrower one that also fits). */
#include <stdint.h>
#include <string.h>

#include "../../nanorq_amd/csrc/obj_body.h"

template <typename W>
static void run(const obj_lay *l) {
  for (uint32_t b = 0; b < l->Z; b++) {
    if (l->to_obj && !((l->mask[b >> 5] >> (b & 31u)) & 1u)) continue;
    const uint32_t nw = obj_windows(l, b), per = OBJ_WG * OBJ_UNROLL;
    for (uint32_t g = 0; g * per < nw; g++)
      for (uint32_t t = 0; t < OBJ_WG; t++) obj_move<W>(l, b, g * per + t, OBJ_WG);
  }
}

extern "C" {

/* prm = {T, Z, ZL, KL, KS, NL, TL, NS, TS}; V 0 = the library's choice; mask: 8 words (rows -> object).  Returns the width used,
 * or -1 if V does not fit. */
int emu_obj_layout(const uint32_t *prm, uint8_t *obj, uint64_t F, uint8_t *rows, uint32_t to_obj, const uint32_t *mask, uint32_t V) {
  obj_lay l;
  memset(&l, 0, sizeof(l));
  l.obj = obj; l.rows = rows; l.F = F;
  l.T = prm[0]; l.Z = prm[1]; l.ZL = prm[2]; l.KL = prm[3]; l.KS = prm[4]; l.NL = prm[5]; l.TL = prm[6]; l.NS = prm[7]; l.TS = prm[8];
  l.to_obj = to_obj;
  l.obj_vec = ((uintptr_t)obj & 15u) == 0;
  if (mask) memcpy(l.mask, mask, sizeof(l.mask));
  const uint32_t best = obj_width(&l);
  if (V == 0) V = best;
  if (V > best || (V & (V - 1u))) return -1;
  switch (V) {
    case 16: run<tx_u128>(&l); break;
    case 8: run<uint64_t>(&l); break;
    case 4: run<uint32_t>(&l); break;
    case 2: run<uint16_t>(&l); break;
    default: run<uint8_t>(&l); break;
  }
  return (int)V;
}

} /* extern "C" */
