/*
 * wave_emu.h -- the lanes of a wave in step, for a CPU emulation that runs them one after the other (TEST SUPPORT ONLY).
 *
 * On the device NRQ_WAVE_ANY(x) is a ballot: true in every lane when x holds in one, so a loop under it runs in EVERY lane as long
 * as ONE lane needs it -- ph_store's fast form reads a second trip of a one-entry list when another lane's list has 33 entries.
 * Include this BEFORE solve_body.h: NRQ_WAVE_ANY then asks wave_any(), and wave_in_step() gives it the wave's answer without
 * threads: the k-th ballot of a wave is the OR of what its lanes say at their k-th ballot (control flow under ballots is the same
 * in all lanes), found one ballot per round -- every lane runs with the answers known so far and stops, by a longjmp, at the
 * first ballot beyond them, where it leaves its own word (the phase functions hold nothing with a destructor).  A lane therefore runs the phase several times; the phase must not mind
 * (ph_store reads the image and the lists and writes what it computed: the same bytes every time).
 */
#ifndef NRQ_WAVE_EMU_H
#define NRQ_WAVE_EMU_H

#include <setjmp.h>

#include <cstddef>
#include <vector>

struct WaveTape {
  std::vector<char> known; /* answers of the ballots found so far */
  size_t at = 0;           /* ballots the running lane has asked */
  bool word = false;       /* OR of the lanes' words at ballot known.size() */
  jmp_buf stop;            /* where a lane that asks beyond `known` goes */
};
static WaveTape *g_wave_tape = nullptr; /* nullptr: no wave in step, a lane's own word is the answer */

static inline bool wave_any(bool x) {
  WaveTape *w = g_wave_tape;
  if (!w) return x;
  if (w->at < w->known.size()) return w->known[w->at++] != 0;
  w->word = w->word || x;
  longjmp(w->stop, 1);
}
#define NRQ_WAVE_ANY(x) wave_any(x)

/* lane(l) for l = 0 .. lanes - 1 with wave-wide ballots; returns the ballots the wave took */
template <class F> static size_t wave_in_step(unsigned lanes, F lane) {
  WaveTape w;
  g_wave_tape = &w;
  for (;;) {
    volatile bool stopped = false;
    w.word = false;
    for (volatile unsigned l = 0; l < lanes; l = l + 1) {
      w.at = 0;
      if (setjmp(w.stop) == 0) lane(l);
      else stopped = true;
    }
    if (!stopped) break;
    w.known.push_back(w.word ? 1 : 0);
  }
  g_wave_tape = nullptr;
  return w.known.size();
}

#endif /* NRQ_WAVE_EMU_H */
