// The transforms' launch schedule (ntt_plan, myzkp_amd/csrc/mzk_ntt_plan.h) run on the host for tests/test_hostcheck_ntt_plan.py.
// Stand-alone: reads "fid logn batch large_fr large_m128 m128_two_wg" lines from the file given as argv[1] (-2 = the knob's default) and
// prints, per line,
//   P fid logn batch large_fr large_m128 m128_two_wg  err geo large nlev lg0 lg1 lg2 lg3 tmp_bytes lds_attr nsteps
//     { kind lgn lgM lgc lgr lg_rows total_rows grid block lds wt } x nsteps
// then the geometries ("G id tl nt maxlv twg wpe"), the default knobs ("K ...") and "ok <lines>".  Built with -fsanitize=address,undefined.
#include <inttypes.h>
#include <stdio.h>
#include "../../myzkp_amd/csrc/mzk_ntt_plan.h"

using namespace mzk;

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ntt_plan_shim cases.txt\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int fid, lfr, lm, twg;
  unsigned logn;
  uint64_t batch;
  size_t lines = 0;
  while (fscanf(f, "%d %u %" SCNu64 " %d %d %d", &fid, &logn, &batch, &lfr, &lm, &twg) == 6) {
    NttKnobs k;
    if (lfr != -2) k.large_fr = lfr;
    if (lm != -2) k.large_m128 = lm;
    if (twg != -2) k.m128_two_wg = twg;
    const NttSchedule S = ntt_plan(fid, logn, (size_t)batch, k);
    if (S.nsteps < 0 || S.nsteps > 4 || (S.err == MZK_OK && S.nsteps != S.li.nlev)) { fprintf(stderr, "step count %d out of range\n", S.nsteps); return 1; }
    if (S.err != MZK_OK) fprintf(stderr, "fid %d logn %u batch %" PRIu64 ": %s\n", fid, logn, batch, S.msg);
    printf("P %d %u %" PRIu64 " %d %d %d  %d %d %d %d %d %d %d %d %zu %d %d", fid, logn, batch, lfr, lm, twg, S.err, S.geo, (int)S.large, S.li.nlev, S.li.lg[0],
           S.li.lg[1], S.li.lg[2], S.li.lg[3], S.tmp_bytes, (int)S.lds_attr, S.nsteps);
    for (int i = 0; i < S.nsteps; i++) {
      const NttStep& s = S.steps[i];
      printf("  %d %d %d %d %d %d %zu %u %u %zu %d", s.kind, s.lgn, s.lgM, s.lgc, s.lgr, s.lg_rows, s.total_rows, s.grid, s.block, s.lds, (int)s.wt);
    }
    printf("\n");
    lines++;
  }
  fclose(f);
  for (int id = 0; id < 5; id++) printf("G %d %d %d %d %d %d\n", id, NTT_GEOS[id].tl, NTT_GEOS[id].nt, NTT_GEOS[id].maxlv, (int)NTT_GEOS[id].twg, NTT_GEOS[id].wpe);
  const NttKnobs d;
  printf("K %d %d %d %d %d %d %d\n", d.large_fr, d.large_m128, d.m128_two_wg, d.wt_lo, d.wt_hi_fr, d.wt_hi_m128, d.wt_mask);
  printf("ok %zu\n", lines);
  return 0;
}
