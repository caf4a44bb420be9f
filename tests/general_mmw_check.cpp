// Which kernels run the per-step moment matching of tests/general_envelope_cases.py's cases: pm_mmw_ok of
// prob_mbrl_amd/csrc/pmbrl_mm_wide.h (plan_layout: mm_wide) against what the table's MM_PER_STEP_WIDE says, on the host
// side of the header alone -- no device code is built or run.  Reads "M D flags wide" lines from standard input.
// Exit status 0: every line agrees (and there was one).
#include <cstdio>

#include "pmbrl_mm_wide.h"

int main() {
  int M, D, flags, want, n = 0, bad = 0;
  while (scanf("%d %d %d %d", &M, &D, &flags, &want) == 4) {
    ++n;
    const bool got = pm_mmw_ok(M, D, (unsigned)flags);
    if (got != (want != 0)) {
      ++bad;
      printf("M %d D %d flags %d: pm_mmw_ok says %d (%zu B of LDS), the table %d\n", M, D, flags, (int)got,
             pm_mmw_lds_bytes(M, D, true), want);
    }
  }
  printf("%d groups, %d disagree\n", n, bad);
  return n > 0 && bad == 0 ? 0 : 1;
}
