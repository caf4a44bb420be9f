// The LDS figures of tests/general_envelope_cases.py against the general family's map (prob_mbrl_amd/csrc/pmbrl_lds_map.h:
// pm_lds_map), host compiler alone -- a sibling of tests/lds_map_check.cpp.  Reads one line per distinct plan of the table
// from standard input, "R LD D U RT mm_d in_place bytes", evaluates the map and compares its total with `bytes`; also
// checks that the regions follow each other inside the total.  Exit status 0: every line agrees (and there was one).
#include <cstdio>

#include "pmbrl_lds_map.h"

int main() {
  int R, LD, D, U, RT, mmd, ip, n = 0, bad = 0;
  long want;
  while (scanf("%d %d %d %d %d %d %d %ld", &R, &LD, &D, &U, &RT, &mmd, &ip, &want) == 8) {
    ++n;
    const PmLdsMap m = pm_lds_map(0, R, LD, D, U, RT, mmd, ip != 0);
    const long got = (long)m.total * (long)sizeof(float);
    const bool ordered = m.bufA == 0 && m.bufB >= m.bufA && m.xa == m.bufB + R * LD && m.xb > m.xa && m.av > m.xb &&
                         m.gad > m.av && m.rr > m.gad && m.gr > m.rr && m.part > m.gr && m.mm >= m.part &&
                         m.total >= m.mm && m.mm % 4 == 0 && (ip ? m.bufB == m.bufA && !m.has_part : m.bufB == R * LD);
    if (got != want || !ordered) {
      ++bad;
      printf("R %d LD %d D %d U %d RT %d mm_d %d in-place %d: the map says %ld B, the table %ld B%s\n", R, LD, D, U, RT, mmd,
             ip, got, want, ordered ? "" : " (regions out of order)");
    }
  }
  printf("%d plans, %d disagree\n", n, bad);
  return n > 0 && bad == 0 ? 0 : 1;
}
